"""What every net with a fused C-ABI forward carries: the flat device copy of its (transposed) weights (``_WeightPack``: allocated
once, rewritten in place, section by section; ``sync_weights()``), ``_Stacked`` for the hop-by-hop groups in it, the mixin of
the acting forwards (``_Acting``: the sampler's Philox stream, the policy-step counter, the output buffers) and ``_as_dev`` for
the numpy-facing entry points.  No counterpart in the reference: this is the host side of the weight structs of include/commarl.h.
"""
import ctypes as C

import numpy as np
import torch

from .. import _lib as L


def _as_dev(x, device):
    if x is None:
        return None
    if not torch.is_tensor(x):
        x = torch.as_tensor(np.asarray(x), dtype=torch.float32)
    return x.to(device=device, dtype=torch.float32)


class _Stacked(list):
    """Equal-shape parameters that the flat weight copy stores back to back (what torch.stack would give, without its launch)."""

    def numel(self):
        return sum(t.numel() for t in self)


class _WeightPack:
    """Flat device copy of a net's (transposed) weights for the fused C-ABI kernels; subclasses list the
    tensors in ``_pack_tensors()``."""
    _pack_sig, _pack, _pack_stale, _train_fwd, _train_fwd_wave, _pack_fresh = None, None, False, False, False, 0

    def _pack_tensors(self):
        raise NotImplementedError

    def _packed(self):
        """Flat contiguous device copy of the (transposed) weights.  Allocated once; when a parameter
        changed (optimizer step / load_state_dict) the SAME buffer is rewritten in place, so device
        pointers - and any hipGraph that captured them - stay valid."""
        sig = tuple((p.data_ptr(), p._version) for p in self.parameters())
        # a training forward (_FusedNetFn sets _train_fwd around its launch) reads the f16-split fragments only: between two optimiser steps just that section is
        # refreshed (cm_*_pack_sections); the rest goes stale and is packed - with the range check - by the next no-grad user
        # (sync_weights() before a rollout, evaluate_nograd, act_device)
        need = (L.PACK_F16 | (L.PACK_WAVE if self._train_fwd_wave else 0)) if self._train_fwd else L.PACK_ALL
        if sig == self._pack_sig and not (need & 7 & ~self._pack_fresh):     # every section this user reads is current
            return self._pack[1]
        with torch.no_grad():
            ts = self._pack_tensors()
            if self._pack is None or self._pack[0].device != next(self.parameters()).device:
                offs, off = {}, 0
                for k, v in ts.items():
                    if v is None:
                        offs[k] = None
                        continue
                    offs[k] = (off, v.numel())
                    off += (v.numel() + 3) & ~3                 # keep every tensor 16-byte aligned
                buf = torch.zeros(off, dtype=torch.float32, device=next(self.parameters()).device)
                base = buf.data_ptr()
                ptrs = {k: (None if o is None else base + 4 * o[0]) for k, o in offs.items()}
                self._pack = (buf, ptrs, offs)
            buf, ptrs, offs = self._pack
            self._flat_copy(ts, buf, offs)
            same = sig == self._pack_sig
            self._pack_sig = None                               # a refused pack (cm_*_pack: weight outside the f16 range) is retried
            self._after_pack(self._pack[1], need)
            self._pack_fresh = (need & 7) | (self._pack_fresh if same else 0)
            self._pack_sig, self._pack_stale = sig, self._pack_fresh != 7
        return self._pack[1]

    def _flat_copy(self, ts, buf, offs):
        """Every tensor of `ts` into its slot of the flat buffer.  On the GPU: ONE launch (cm_multi_copy_t) for all the plain
        parameters and transposed weight views (`weight.t()`: the source is the parameter itself, the kernel transposes; a
        _Stacked group entry by entry); anything else through the framework's copy."""
        plain = []
        for k, v in ts.items():
            if v is None:
                continue
            o, n = offs[k]
            if isinstance(v, _Stacked):                      # the stack's members one after the other
                parts, po = [], o
                for t in v:
                    parts.append((t, po, t.numel()))
                    po += t.numel()
            else:
                parts = [(v, o, n)]
            for v, o, n in parts:
                self._flat_copy_one(v, buf[o:o + n], n, plain, buf)
        if plain:
            m = len(plain)
            src = (C.c_void_p * m)(*[t[0] for t in plain])
            dstp = (C.c_void_p * m)(*[t[1] for t in plain])
            rows = (C.c_int32 * m)(*[t[2] for t in plain])
            cols = (C.c_int32 * m)(*[t[3] for t in plain])
            tr = (C.c_int32 * m)(*[t[4] for t in plain])
            L.run("cm_multi_copy_t", m, src, dstp, rows, cols, tr, device=buf.device)

    @staticmethod
    def _flat_copy_one(v, dst, n, plain, buf):
        base = v._base if (v.dim() == 2 and v._base is not None and not v.is_contiguous()) else None
        if (buf.is_cuda and v.dtype == torch.float32 and v.dim() <= 2 and len(plain) < 40
                and (v.is_contiguous() or (base is not None and base.is_contiguous() and base.dim() == 2
                                           and base.shape == v.shape[::-1] and v.data_ptr() == base.data_ptr()))):
            if v.is_contiguous():
                plain.append((v.data_ptr(), dst.data_ptr(), 1, n, 0))
            else:                                            # v = base.t(): dst[c][r] = base[r][c]
                plain.append((base.data_ptr(), dst.data_ptr(), base.shape[0], base.shape[1], 1))
        else:
            dst.copy_(v.detach().to(torch.float32).reshape(-1))

    def _after_pack(self, ptrs, sections=15):
        """Hook: derived device-side layouts (the matrix-core operand pack) are rebuilt here."""

    def sync_weights(self):
        """Refresh the fused kernels' weight pack (call after an optimizer step, outside graphs)."""
        self._packed()

    def grad_norm(self):
        return float(np.sqrt(np.sum([p.grad.norm(2).item() ** 2 for p in self.parameters() if p.grad is not None])))

    def reset(self, dones=None):
        return

    @property
    def recurrent(self):
        return False


class _Acting:
    """What the acting forwards (act_device) of the Comm-DP policy and the row-MLP policies share: the sampler's Philox stream,
    the policy-step counter and the output buffers."""

    def set_rng(self, seed, env_id_offset=0):
        """Philox stream of the action sampler: counter (env id, policy step, site 7, agent)."""
        self.seed, self.env_id_offset = int(seed), int(env_id_offset)

    def _next_step(self):
        """This policy's own step counter (what act_device uses when it is given no policy_step), which then advances."""
        self._policy_step += 1
        return self._policy_step - 1

    def _act_outputs(self, S, dev, want_actions, want_probs, want_attn, out_actions, out_probs, out_attn):
        """(actions int32 [S,N], probs [S,N,A], attn [S,N,N]) on `dev`: the caller's buffer, else a new one where wanted, else None."""
        if dev.type != "cuda":
            raise L.CommarlError("the rollout forward is a HIP kernel: inputs must be CUDA tensors (no CPU fallback)")
        N = self._n_agents
        if out_actions is None and want_actions:
            out_actions = torch.empty(S, N, dtype=torch.int32, device=dev)
        if out_probs is None and want_probs:
            out_probs = torch.empty(S, N, self._action_dim, dtype=torch.float32, device=dev)
        if out_attn is None and want_attn:
            out_attn = torch.empty(S, N, N, dtype=torch.float32, device=dev)
        return out_actions, out_probs, out_attn
