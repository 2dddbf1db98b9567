"""What the tests of the dense-layer kernels (csrc/cm_linear.hip, cm_linear_bwd.hip, cm_linear_wgrad.hip) share: no test in here,
no GPU, nothing of com_marl_amd.

  CASES     (name, entry, R, K, O, layout, act, bias/db, dx, dy2, route, note, opts), written by hand from the dispatch code: the note
            names the branch or boundary a case is there for and the function that owns it.  entry: fwd (cm_linear_act_forward),
            bwd (cm_linear_act_backward and its _ex / _det / _ex_det forms), wgrad (cm_linear_wgrad / _det, with P = K, Q = O and
            colsum_a in the bias/db column).  opts: "" | "sat" (saturated outputs) | "z1e-2" / "z1e-3" (forward pre-activations of
            that size) | "off" (x, dy, dy2, y - a, b of wgrad - each one float into a larger allocation) | "offx" (x alone)
  route     where a call lands, restated in Python from the dispatch code (see its docstring)
  build     the float32 inputs of a case, seeded by its name; reference the float64 answers (ref64) - both cached and read-only
  ref64     y, or dz -> dx, dW in the weight's own layout, db, or c / colsum_a, from the float32 inputs widened to float64
  emu32     the same in float32 with the kernels' summation structure: products and sums in float32, one partial per 64-row chunk,
            chunks summed per workgroup of the forward / generic grid min(chunks, 512), the workgroup partials merged in float32.
            What float32 ALONE does to a case, never a reference
  judge     {quantity: (strict, applied)} of an output against ref64 with tests/test_backward_kernels_f64._metric:
            max|got - ref| / max|ref| per tensor, dx and y also per row (a row's scale floored at 1e-3 of the tensor's); bar TAU = 1e-5.
            The applied ratio differs from the strict one for ONE quantity, the forward's tanh output, whose bar is
            max(TAU scale, 2e-7) absolute: 2e-7 is what cm_linear.hip documents for tanh_exact (1 - 2 / (exp2(c x) + 1) cancels for
            small |x|: ~1.8e-7 absolute at any scale).  An initial content `init` of the accumulated outputs is added to the reference
  term_sums the sum of the magnitudes of the terms of every accumulated element: the bound on any partial sum of it
  controls  wrong answers built in float64 from the reference, each with whether it COINCIDES with the right one for that case"""
import functools
import zlib

import numpy as np
import torch

from tests.test_backward_kernels_f64 import _metric

TAU = 1e-5
TANH_ABS = 2e-7                      # cm_linear.hip: tanh_exact's documented absolute error
ROWS = 64                            # lin::ROWS, lin2::ROWS, WG_ROWS
GRID_CAP = 512                       # forward, generic backward, wgrad: min(chunks, 512) workgroups
N_CU = 256                           # MI355X compute units (cm::cu_count on the test machine), for the notes on the stream grid only
ROW_COUNTS = (1, 63, 64, 65, 2555, 32833, 144705)
F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------------------------------
# where a call lands
# ------------------------------------------------------------------------------------------------------------------------------
def _tiles(w):
    return (w + 15) // 16


def _maxt(nt):
    """linear_bwd_generic / linear_wgrad: the accumulator tiles per wave are the MAXT instantiation that holds ceil(NT / 4)."""
    per_wave = (nt + 3) // 4
    return next(m for m in (1, 2, 4, 8, 16) if per_wave <= m)


def _vec(w, aligned, lo=16):
    """lin::stage (lo = 16) / stage_rows (lo = 4): float4 loads for a power-of-two number of float4s per row, aligned pointers."""
    return aligned and w % 4 == 0 and (w // 4) & (w // 4 - 1) == 0 and lo <= w <= 128


STREAM_W = (32, 64, 128)
STREAM_RELU = ((64, 32), (128, 64))          # CM_B2_RELU in bwd_stream
RAGGED_RELU_O = 128                          # CM_RG_RELU in bwd_stream: the ragged first layer into 128


def stream_lds(K16, O, WO, act, dy2):
    """lin2::launch: two buffers of dz | x (| obs) tiles, the y tile, the dy2 tile - refused above 160 KiB."""
    return (2 * ROWS * (K16 + O + WO) + (ROWS * O if act else 0) + (ROWS * O if dy2 else 0)) * 4


def route(entry, K, O, layout=0, act=0, dx=True, dy2=False, aligned=True, x_aligned=None):
    """Restates, for one call, which kernel the host code picks.  Update it with:
      cm_linear_act_forward + lin::fwd_kernel (cm_linear.hip)   tile split OT = ceil(O / 16): OT < 4 -> wave % OT, row tiles from
                                                               wave / OT in steps of 4 / OT; else ceil(OT / 4) column tiles per wave
      bwd_stream (cm_linear_bwd.hip)                           its two predicates in order - the ragged first layer (K not a stream
                                                               width, O one, dx NULL, layout 0, dy / dy2 / y 16-byte and x 4-byte
                                                               aligned; ReLU only into O = 128), then the stream kernel (both widths
                                                               in 32 / 64 / 128, not 128 x 128, everything 16-byte aligned, layout 1
                                                               only 64 x 64, ReLU only 64 -> 32 and 128 -> 64) - and lin2::launch's
                                                               160 KiB refusal
      linear_bwd_generic (cm_linear.hip), linear_wgrad (cm_linear_wgrad.hip)   MAXT from NT = OT KT (PT QT)
    aligned: dy, dy2, y (and x unless x_aligned says otherwise) are 16-byte aligned; x is always 4-byte aligned.
    -> 'fwd/OT<n>/<vec|sca>', 'stream/<K>x<O>/L<layout>/act<a>', 'ragged/kt<n>x<O>/act<a>', 'generic/MAXT<m>/<why>' with why in
    width, 128x128, unaligned, layout1, no-relu, ragged-no-relu, lds; 'wgrad/MAXT<m>/<vec|sca><vec|sca>' (staging of a, b)."""
    xa = aligned if x_aligned is None else x_aligned
    if entry == "fwd":
        return f"fwd/OT{_tiles(O)}/{'vec' if _vec(K, xa) else 'sca'}"
    if entry == "wgrad":
        return f"wgrad/MAXT{_maxt(_tiles(K) * _tiles(O))}/{'vec' if _vec(K, xa, 4) else 'sca'}{'vec' if _vec(O, aligned, 4) else 'sca'}"
    assert entry == "bwd"
    generic = f"generic/MAXT{_maxt(_tiles(K) * _tiles(O))}/"
    ok = lambda v: v in STREAM_W                                   # noqa: E731
    if not ok(K) and ok(O) and not dx and layout == 0 and aligned:
        kt = 2 if K <= 32 else (4 if K <= 64 else 8)
        if act == 2 and O != RAGGED_RELU_O:
            return generic + "ragged-no-relu"
        if stream_lds(16 * kt, O, 0, act, dy2) > 160 * 1024:
            return generic + "lds"
        return f"ragged/kt{kt}x{O}/act{act}"
    if not ok(K) or not ok(O):
        return generic + "width"
    if K == 128 and O == 128:
        return generic + "128x128"
    if not (aligned and xa):
        return generic + "unaligned"
    if layout == 1 and not (K == 64 and O == 64):
        return generic + "layout1"
    if act == 2 and (layout == 1 or (K, O) not in STREAM_RELU):
        return generic + "no-relu"
    if stream_lds(K, O, 0, act, dy2) > 160 * 1024:
        return generic + "lds"
    return f"stream/{K}x{O}/L{layout}/act{act}"


def stream_grid(R):
    """lin2::launch's grid on a device of N_CU compute units."""
    chunks = (R + ROWS - 1) // ROWS
    return max(1, min(chunks, N_CU, max(1, int(np.floor(np.sqrt(29.0 * chunks) + 0.5)))))


def route_of(c):
    al = c.opts != "off"
    return route(c.entry, c.K, c.O, c.layout, c.act, c.dx, c.dy2, aligned=al, x_aligned=al and c.opts != "offx")


# ------------------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------------------
class Case(tuple):
    FIELDS = ("name", "entry", "R", "K", "O", "layout", "act", "bias", "dx", "dy2", "route", "note", "opts")

    def __getattr__(self, k):
        try:
            return self[self.FIELDS.index(k)]
        except ValueError:
            raise AttributeError(k) from None


def _name(entry, R, K, O, layout, act, bias, dx, dy2, opts):
    s = f"{entry}-R{R}-{K}x{O}-L{layout}a{act}"
    if entry == "fwd":
        s += "" if bias else "-nob"
    elif entry == "bwd":
        s += ("" if bias else "-nodb") + ("" if dx else "-nodx") + ("-dy2" if dy2 else "")
    else:
        s = f"wgrad-R{R}-{K}x{O}" + ("" if bias else "-nocs")
    return s + (f"-{opts}" if opts else "")


def F(R, K, O, layout, act, bias, rt, note, opts=""):
    return Case((_name("fwd", R, K, O, layout, act, bias, False, False, opts), "fwd", R, K, O, layout, act, bias, False, False, rt, note, opts))


def B(R, K, O, layout, act, db, dx, dy2, rt, note, opts=""):
    return Case((_name("bwd", R, K, O, layout, act, db, dx, dy2, opts), "bwd", R, K, O, layout, act, db, dx, dy2, rt, note, opts))


def G(R, P, Q, colsum, rt, note, opts=""):
    return Case((_name("wgrad", R, P, Q, 0, 0, colsum, False, False, opts), "wgrad", R, P, Q, 0, 0, colsum, False, False, rt, note, opts))


_FWD = [
    F(1, 1, 1, 0, 0, True, "fwd/OT1/sca", "one row, K = O = 1: fwd_kernel's OT = 1 split (rt_start = wave, rt_step = 4)"),
    F(65, 1, 1, 0, 1, True, "fwd/OT1/sca", "a second chunk of one row; tanh_exact"),
    F(63, 5, 3, 0, 1, True, "fwd/OT1/sca", "one ragged chunk; widths below 16 on both sides"),
    F(64, 3, 5, 0, 2, True, "fwd/OT1/sca", "exactly one chunk; ReLU (z < 0 ? 0 : z)"),
    F(32833, 5, 3, 0, 1, True, "fwd/OT1/sca", "514 chunks on cm_linear_act_forward's 512-workgroup cap, a one-row tail"),
    F(65, 16, 16, 0, 1, True, "fwd/OT1/vec", "K = 16: lin::stage's vector branch with ni = 1"),
    F(2555, 17, 15, 0, 1, True, "fwd/OT1/sca", "one past / one short of a tile: KT = 2 with 15 padded k, 15 live columns of 16"),
    F(2555, 64, 32, 0, 2, True, "fwd/OT2/vec", "fwd_kernel's OT = 2 split (ct0 = wave % 2, rt_start = wave / 2, rt_step = 2)"),
    F(65, 20, 40, 0, 1, True, "fwd/OT3/sca", "OT = 3: wave 3 recomputes column tile 0 from row tile 1 (fwd_kernel); K = 20 a multiple "
                                            "of 4 on the scalar branch of lin::stage"),
    F(65, 96, 48, 0, 1, True, "fwd/OT3/sca", "OT = 3; K = 96: 24 float4s, not a power of two -> scalar branch of lin::stage"),
    F(2555, 40, 60, 0, 2, False, "fwd/OT4/sca", "OT = 4: the first split with one column tile per wave, the last 12 wide; no bias"),
    F(2555, 80, 80, 0, 1, True, "fwd/OT5/sca", "OT = 5: two tiles per wave, wave 2's second is dead, wave 3 idle (fwd_kernel's live)"),
    F(65, 48, 96, 0, 0, True, "fwd/OT6/sca", "OT = 6, identity: waves 0..2 two tiles, wave 3 none"),
    F(2555, 7, 100, 0, 1, True, "fwd/OT7/sca", "OT = 7: wave 3's first tile is the last live one (4 columns), its second dead"),
    F(65, 100, 7, 0, 1, True, "fwd/OT1/sca", "KT = 7 into 7 columns"),
    F(65, 112, 128, 0, 1, True, "fwd/OT8/sca", "OT = 8 (both tiles of every wave); K = 112 = 28 float4s on the scalar branch"),
    F(32833, 128, 128, 0, 1, True, "fwd/OT8/vec", "the widest layer on the 512-workgroup cap with a one-row tail; ni = 8 in lin::stage"),
    F(65, 48, 96, 1, 0, True, "fwd/OT6/sca", "layout 1 ([in][out]) in w_at"),
    F(65, 48, 96, 1, 1, False, "fwd/OT6/sca", "layout 1, tanh, no bias"),
    F(65, 5, 3, 1, 1, True, "fwd/OT1/sca", "layout 1 below a tile"),
    F(65, 5, 3, 1, 0, False, "fwd/OT1/sca", "layout 1 below a tile, no bias"),
    F(65, 64, 64, 0, 2, True, "fwd/OT4/vec", "ReLU at the graph-convolution width"),
    F(65, 32, 128, 0, 2, True, "fwd/OT8/vec", "ReLU, ni = 2 in lin::stage"),
    F(1, 64, 64, 0, 1, True, "fwd/OT4/vec", "one row on the vector branch (63 zero rows staged)"),
    F(2555, 64, 64, 0, 1, True, "fwd/OT4/vec", "tanh_exact where 1 - 2 / (exp2 + 1) cancels: pre-activations of 1e-2", "z1e-2"),
    F(2555, 64, 64, 0, 1, True, "fwd/OT4/vec", "tanh_exact where 1 - 2 / (exp2 + 1) cancels: pre-activations of 1e-3", "z1e-3"),
    F(65, 64, 64, 0, 1, True, "fwd/OT4/sca", "x one float into its allocation: lin::stage must take its scalar branch", "off"),
    F(65, 32, 128, 0, 1, True, "fwd/OT8/sca", "x one float into its allocation", "off"),
    F(65, 21, 128, 0, 1, True, "fwd/OT8/sca", "the observation width, x one float into its allocation", "off"),
]

_GENERIC = [
    B(1, 1, 1, 0, 1, True, True, False, "generic/MAXT1/width", "one row, K = O = 1: lin::bwd_kernel's KT = 1 dx split"),
    B(63, 5, 3, 0, 1, True, True, True, "generic/MAXT1/width", "one ragged chunk, widths below 16 on both sides, dy2"),
    B(64, 3, 5, 0, 2, True, True, False, "generic/MAXT1/width", "exactly one chunk; relu_bwd's select"),
    B(32833, 5, 3, 0, 1, True, True, False, "generic/MAXT1/width", "514 chunks on linear_bwd_generic's 512 cap, one-row tail"),
    B(65, 16, 16, 0, 1, True, True, True, "generic/MAXT1/width", "16 x 16: lin::stage's vector branch with ni = 1, dy2 and y as float4"),
    B(2555, 17, 15, 0, 1, True, True, False, "generic/MAXT1/width", "NT = 2: waves 2, 3 recompute tile 0 (aoff / boff of idle slots)"),
    B(65, 20, 40, 0, 1, True, True, False, "generic/MAXT2/width", "NT = 6 -> MAXT 2; KT = 2 dx split (kt0 = wave % 2, rt_step 2)"),
    B(65, 100, 7, 0, 1, True, True, False, "generic/MAXT2/width", "NT = 7 -> MAXT 2; nkt = 2 with wave 3's second k tile dead"),
    B(2555, 7, 100, 0, 2, True, True, False, "generic/MAXT2/width", "NT = 7, ReLU; KT = 1"),
    B(2555, 40, 60, 0, 2, True, True, True, "generic/MAXT4/width", "NT = 12 -> MAXT 4; KT = 3: wave 3 recomputes k tile 0 from row tile 1"),
    B(65, 40, 60, 0, 1, True, False, False, "generic/MAXT4/width", "dx NULL off the ragged kernel's widths (O = 60)"),
    B(65, 80, 80, 0, 1, True, True, False, "generic/MAXT8/width", "NT = 25 -> MAXT 8 (two workgroups per CU by its launch bounds)"),
    B(65, 48, 96, 0, 0, True, True, True, "generic/MAXT8/width", "NT = 18; identity with dy2 (stage<0> with src2)"),
    B(65, 96, 48, 0, 1, True, True, False, "generic/MAXT8/width", "NT = 18 the other way; both widths multiples of 4 on the scalar branch"),
    B(65, 112, 128, 0, 1, True, True, False, "generic/MAXT16/width", "NT = 56 -> MAXT 16"),
    B(32833, 128, 128, 0, 1, True, True, True, "generic/MAXT16/128x128", "the one pair of stream widths bwd_stream refuses; NT = 64; the "
                                                                      "512 cap with a one-row tail"),
    B(65, 48, 96, 1, 1, True, True, False, "generic/MAXT8/width", "layout 1: (P, Q) = (K, O), As / Bs swapped in lin::bwd_kernel"),
    B(65, 48, 96, 1, 0, False, True, True, "generic/MAXT8/width", "layout 1, identity, db NULL"),
    B(65, 5, 3, 1, 1, True, True, False, "generic/MAXT1/width", "layout 1 below a tile"),
    B(65, 5, 3, 1, 0, False, True, False, "generic/MAXT1/width", "layout 1 below a tile, db NULL"),
    B(65, 32, 64, 1, 1, True, True, False, "generic/MAXT2/layout1", "layout 1 at stream widths other than 64 x 64 (bwd_stream's refusal)"),
    B(65, 64, 64, 0, 2, True, True, False, "generic/MAXT4/no-relu", "ReLU at a stream shape without a ReLU build (CM_B2 returns 1)"),
    B(2555, 32, 128, 0, 2, True, True, True, "generic/MAXT4/no-relu", "ReLU at 32 -> 128: no ReLU build"),
    B(65, 64, 64, 1, 2, True, True, False, "generic/MAXT4/no-relu", "ReLU on the layout-1 build (CM_B2, not CM_B2_RELU)"),
    B(65, 31, 64, 0, 2, True, False, False, "generic/MAXT2/ragged-no-relu", "ReLU first layer into 64: CM_RG returns 1"),
    B(65, 127, 128, 0, 1, True, False, True, "generic/MAXT16/lds", "ragged kt 8 into 128 with tanh AND dy2: 192 KiB, lin2::launch refuses"),
    B(2555, 40, 60, 0, 1, True, True, False, "generic/MAXT4/width", "saturated tanh outputs: y = +-1 exactly gives dz = 0 exactly", "sat"),
    B(2555, 40, 60, 0, 2, True, True, True, "generic/MAXT4/width", "dead ReLU units: y = 0 exactly gives dz = 0 exactly", "sat"),
    B(65, 64, 64, 0, 1, True, True, True, "generic/MAXT4/unaligned", "x, dy, dy2, y one float in: bwd_stream's alignment test sends it "
                                                                    "here, lin::stage must take its scalar branch", "off"),
    B(65, 32, 128, 0, 1, True, True, True, "generic/MAXT4/unaligned", "the same at 32 -> 128", "off"),
    B(65, 21, 128, 0, 1, True, False, True, "generic/MAXT4/width", "first layer with dy, dy2, y one float in: the ragged predicate fails",
      "off"),
]

_STREAM = [
    B(2555, 32, 32, 0, 1, True, True, True, "stream/32x32/L0/act1", "KT 2 / OT 2; 40 chunks on 34 workgroups, 6 of them two chunks, ragged "
                                                                   "last chunk (lin2::launch's sqrt(29 chunks) grid)"),
    B(65, 32, 64, 0, 1, True, True, False, "stream/32x64/L0/act1", "KT 2 / OT 4, no dy2: finish_tile's ACT branch alone"),
    B(2555, 32, 128, 0, 1, True, False, False, "stream/32x128/L0/act1", "OT 8; dx NULL on the stream kernel (wf never loaded)"),
    B(64, 64, 32, 0, 1, True, True, True, "stream/64x32/L0/act1", "exactly one chunk: no finish_tile zeroing"),
    B(1, 64, 64, 0, 1, True, True, False, "stream/64x64/L0/act1", "one row: the DMA re-reads row 0 for 63 rows, finish_tile zeroes them"),
    B(144705, 64, 64, 0, 1, True, True, True, "stream/64x64/L0/act1", "2262 chunks: the grid is the CU count, ragged tail"),
    B(2555, 64, 128, 0, 1, True, True, True, "stream/64x128/L0/act1", "tanh and dy2 at 64 -> 128: exactly 160 KiB, one float from "
                                                                     "lin2::launch's refusal"),
    B(63, 128, 32, 0, 1, True, False, True, "stream/128x32/L0/act1", "KT 8 / OT 2, dx NULL with dy2, one ragged chunk"),
    B(32833, 128, 32, 0, 1, True, True, True, "stream/128x32/L0/act1", "514 chunks on 122 workgroups; the slab twin's rows = its grid"),
    B(2555, 128, 64, 0, 1, True, True, True, "stream/128x64/L0/act1", "tanh and dy2 at 128 -> 64 (128 KiB): y and dy2 tiles behind two buffers"),
    B(2555, 64, 64, 1, 1, True, True, True, "stream/64x64/L1/act1", "the layout-1 build: db summed per half of the permuted tiling"),
    B(65, 32, 32, 0, 0, True, False, False, "stream/32x32/L0/act0", "identity, nothing to finish but the ragged chunk's zero rows; dx NULL"),
    B(2555, 32, 64, 0, 0, True, True, True, "stream/32x64/L0/act0", "dy2 with act 0: finish_tile's ACT || DY2 branch without a y tile"),
    B(65, 32, 128, 0, 0, True, True, True, "stream/32x128/L0/act0", "OT 8 identity with dy2"),
    B(2555, 64, 32, 0, 0, False, True, False, "stream/64x32/L0/act0", "db NULL on the stream kernel"),
    B(32833, 64, 64, 0, 0, True, True, False, "stream/64x64/L0/act0", "514 chunks on 122 workgroups, one-row tail"),
    B(65, 64, 128, 0, 0, True, False, True, "stream/64x128/L0/act0", "dx NULL with dy2, identity"),
    B(2555, 128, 32, 0, 0, True, True, False, "stream/128x32/L0/act0", "KT 8 / OT 2 identity"),
    B(144705, 128, 64, 0, 0, True, True, True, "stream/128x64/L0/act0", "CU-count grid at the widest input, dy2"),
    B(65, 64, 64, 1, 0, True, False, False, "stream/64x64/L1/act0", "layout 1, identity, dx NULL"),
    B(2555, 64, 32, 0, 2, True, True, True, "stream/64x32/L0/act2", "the Obs-DP head's ReLU build (CM_B2_RELU)"),
    B(1, 64, 32, 0, 2, True, True, False, "stream/64x32/L0/act2", "ReLU build, one row"),
    B(144705, 128, 64, 0, 2, True, True, False, "stream/128x64/L0/act2", "CENT's ReLU build on the CU-count grid"),
    B(2555, 64, 64, 0, 1, True, True, True, "stream/64x64/L0/act1", "saturated tanh outputs in finish_tile: dz = 0 exactly", "sat"),
    B(2555, 64, 32, 0, 2, True, True, False, "stream/64x32/L0/act2", "dead ReLU units in finish_tile: dz = 0 exactly", "sat"),
]

_RAGGED = [
    B(65, 1, 32, 0, 1, True, False, True, "ragged/kt2x32/act1", "K = 1: every tile column but one from zero_word (issue_tile_ragged)"),
    B(1, 33, 32, 0, 1, True, False, False, "ragged/kt4x32/act1", "one row; K = 33, the first width of kt 4"),
    B(2555, 31, 64, 0, 1, True, False, False, "ragged/kt2x64/act1", "K = 31, the last width of kt 2"),
    B(2555, 21, 128, 0, 1, True, False, True, "ragged/kt2x128/act1", "the PP observation into 128: TSPLIT at kt 2"),
    B(32833, 21, 128, 0, 1, True, False, True, "ragged/kt2x128/act1", "TSPLIT on 122 workgroups, one-row tail"),
    B(65, 33, 32, 0, 0, True, False, False, "ragged/kt4x32/act0", "identity first layer, kt 4"),
    B(2555, 48, 64, 0, 1, True, False, True, "ragged/kt4x64/act1", "K = 48: rows happen to be 16-byte aligned, still the dword path"),
    B(65, 53, 128, 0, 1, True, False, False, "ragged/kt4x128/act1", "TSPLIT at kt 4"),
    B(2555, 65, 32, 0, 1, False, False, True, "ragged/kt8x32/act1", "K = 65, the first width of kt 8; db NULL"),
    B(65, 96, 64, 0, 0, True, False, True, "ragged/kt8x64/act0", "K = 96 aligned rows on the dword path, identity with dy2"),
    B(2555, 63, 64, 0, 1, True, False, False, "ragged/kt4x64/act1", "K = 63, the last width of kt 4"),
    B(2555, 127, 128, 0, 1, True, False, False, "ragged/kt8x128/act1", "TSPLIT at kt 8, one zero column; exactly 160 KiB with the y tile"),
    B(65, 127, 128, 0, 0, True, False, True, "ragged/kt8x128/act0", "kt 8 into 128 with dy2 and no y: 160 KiB"),
    B(65, 21, 128, 0, 2, True, False, False, "ragged/kt2x128/act2", "ReLU first layer (CM_RG_RELU) at kt 2"),
    B(2555, 53, 128, 0, 2, True, False, True, "ragged/kt4x128/act2", "ReLU first layer at kt 4 with dy2: 160 KiB"),
    B(65, 127, 128, 0, 2, True, False, False, "ragged/kt8x128/act2", "ReLU first layer at kt 8"),
    B(65, 21, 128, 0, 1, True, False, True, "ragged/kt2x128/act1", "x alone one float in: the ragged kernel asks x for 4 bytes only", "offx"),
]

_WGRAD = [
    G(1, 1, 1, True, "wgrad/MAXT1/scasca", "one row, one element"),
    G(65, 5, 3, True, "wgrad/MAXT1/scasca", "below a tile on both sides, a second chunk of one row"),
    G(64, 4, 8, True, "wgrad/MAXT1/vecvec", "P = 4, Q = 8: stage_rows' float4 branch takes one and two float4s per row"),
    G(65, 4, 8, True, "wgrad/MAXT1/scasca", "the same one float in: stage_rows must take its scalar branch", "off"),
    G(63, 16, 16, True, "wgrad/MAXT1/vecvec", "one ragged chunk, one tile"),
    G(65, 12, 48, True, "wgrad/MAXT1/scasca", "multiples of 4 that are no power-of-two number of float4s; NT = 3"),
    G(2555, 20, 40, True, "wgrad/MAXT2/scasca", "NT = 6 -> MAXT 2"),
    G(2555, 40, 60, False, "wgrad/MAXT4/scasca", "NT = 12 -> MAXT 4, colsum_a NULL"),
    G(65, 64, 64, True, "wgrad/MAXT4/vecvec", "NT = 16, the upper edge of MAXT 4"),
    G(65, 80, 80, True, "wgrad/MAXT8/scasca", "NT = 25 -> MAXT 8"),
    G(65, 112, 96, True, "wgrad/MAXT16/scasca", "NT = 42 -> MAXT 16"),
    G(32833, 128, 128, True, "wgrad/MAXT16/vecvec", "NT = 64 on linear_wgrad's 512 cap, one-row tail"),
    G(65, 128, 5, True, "wgrad/MAXT2/vecsca", "128 x 5: colsum_a over 128 columns (tid < P)"),
    G(65, 128, 5, False, "wgrad/MAXT2/vecsca", "128 x 5, colsum_a NULL"),
    G(2555, 5, 128, True, "wgrad/MAXT2/scavec", "5 x 128: the GCN orientation"),
    G(65, 5, 128, False, "wgrad/MAXT2/scavec", "5 x 128, colsum_a NULL"),
    G(65, 64, 64, True, "wgrad/MAXT4/scasca", "a, b one float in", "off"),
    G(65, 32, 128, True, "wgrad/MAXT4/scasca", "a, b one float in", "off"),
    G(65, 21, 128, True, "wgrad/MAXT4/scasca", "a, b one float in at the observation width", "off"),
]

CASES = _FWD + _GENERIC + _STREAM + _RAGGED + _WGRAD
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES), "case names must be unique"


def group(c):
    """The kernel family a case is filed under (the GPU test's parametrisation)."""
    return c.entry if c.entry != "bwd" else c.route.split("/")[0]


# ------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------
def _tanh32(z):
    with np.errstate(over="ignore"):
        t = np.exp2(z.astype(F32) * F32(2.8853900817779268))
    return (F32(1.0) - F32(2.0) / (t + F32(1.0))).astype(F32)


def _act_of_preact(rng, shape, act):
    z = rng.standard_normal(shape).astype(F32)
    return np.tanh(z.astype(F64)).astype(F32) if act == 1 else np.maximum(z, F32(0))


def draw(c):
    """float32 inputs of a case: x ~ N(0,1), w ~ 0.2 N(0,1) in its own layout, bias ~ 0.1 N(0,1), dy, dy2 ~ N(0,1), y the float32
    tanh / ReLU of a random pre-activation.  'sat': the upper half of y's columns and the first half of its rows are exactly +-1
    (tanh) or 0 (ReLU).  'z1e-2' / 'z1e-3': w and bias scaled so that the pre-activations have that size."""
    rng = np.random.RandomState(zlib.crc32(c.name.encode()) & 0x7FFFFFFF)
    R, K, O = c.R, c.K, c.O
    d = {}
    if c.entry == "wgrad":
        d["a"], d["b"] = rng.standard_normal((R, K)).astype(F32), rng.standard_normal((R, O)).astype(F32)
    else:
        d["x"] = rng.standard_normal((R, K)).astype(F32)
        d["w"] = (0.2 * rng.standard_normal((O, K) if c.layout == 0 else (K, O))).astype(F32)
        if c.entry == "fwd":
            d["bias"] = (0.1 * rng.standard_normal(O)).astype(F32) if c.bias else None
            if c.opts.startswith("z"):
                s = F32(float(c.opts[1:]) / (0.2 * np.sqrt(K)))
                d["w"] = d["w"] * s
                d["bias"] = d["bias"] * s
        else:
            d["dy"] = rng.standard_normal((R, O)).astype(F32)
            d["dy2"] = rng.standard_normal((R, O)).astype(F32) if c.dy2 else None
            d["y"] = _act_of_preact(rng, (R, O), c.act) if c.act else None
            if c.opts == "sat":
                sat = np.sign(rng.standard_normal((R, O))).astype(F32) if c.act == 1 else np.zeros((R, O), F32)
                d["y"][:, O // 2:] = sat[:, O // 2:]
                d["y"][:R // 2] = sat[:R // 2]
    for v in d.values():
        if v is not None:
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def build(name):
    return draw(BY_NAME[name])


# ------------------------------------------------------------------------------------------------------------------------------
# float64 reference
# ------------------------------------------------------------------------------------------------------------------------------
def _w_ko(w, layout):
    """the weight as [K][O], whatever its layout"""
    return w.T if layout == 0 else w


def dz64(c, d):
    dz = d["dy"].astype(F64) + (d["dy2"].astype(F64) if d.get("dy2") is not None else 0.0)
    if c.act == 1:
        dz = dz * (1.0 - d["y"].astype(F64) ** 2)
    elif c.act == 2:
        dz = np.where(d["y"] > 0, dz, 0.0)
    return dz


def ref64(c, d):
    """-> dict of float64 arrays: fwd y; bwd dx (when asked for), dw (the weight's layout), db (when asked for); wgrad c, colsum."""
    if c.entry == "wgrad":
        a, b = d["a"].astype(F64), d["b"].astype(F64)
        out = {"c": a.T @ b}
        if c.bias:
            out["colsum"] = a.sum(0)
        return out
    x, w = d["x"].astype(F64), d["w"].astype(F64)
    if c.entry == "fwd":
        z = x @ _w_ko(w, c.layout)
        if d["bias"] is not None:
            z = z + d["bias"].astype(F64)
        return {"y": np.tanh(z) if c.act == 1 else (np.where(z < 0, 0.0, z) if c.act == 2 else z)}
    dz = dz64(c, d)
    out = {"dw": dz.T @ x if c.layout == 0 else x.T @ dz}
    if c.dx:
        out["dx"] = dz @ _w_ko(w, c.layout).T
    if c.bias:
        out["db"] = dz.sum(0)
    return out


def term_sums(c, d):
    """Per element of each accumulated quantity, the sum over rows of the magnitudes of its terms, sum_r |a_rp| |b_rq| (float64):
    no running value of the kernels' sums - any chunk, workgroup or merge order - exceeds it but by float32 rounding."""
    if c.entry == "wgrad":
        a, b = np.abs(d["a"].astype(F64)), np.abs(d["b"].astype(F64))
        return {"c": a.T @ b, "colsum": a.sum(0)}
    dz, x = np.abs(dz64(c, d)), np.abs(d["x"].astype(F64))
    return {"dw": dz.T @ x if c.layout == 0 else x.T @ dz, "db": dz.sum(0)}


@functools.lru_cache(maxsize=None)
def reference(name):
    r = ref64(BY_NAME[name], build(name))
    for v in r.values():
        v.setflags(write=False)
    return r


# ------------------------------------------------------------------------------------------------------------------------------
# float32 comparator
# ------------------------------------------------------------------------------------------------------------------------------
def _chunked(a):
    R, W = a.shape
    n = (R + ROWS - 1) // ROWS
    p = np.zeros((n * ROWS, W), F32)
    p[:R] = a
    return p.reshape(n, ROWS, W)


def _merge32(part):
    """part [chunks, ...] float32 -> chunk partials summed per workgroup (chunk ch belongs to workgroup ch % grid, in order), the
    workgroup sums then added one by one, all in float32."""
    n = part.shape[0]
    g = min(n, GRID_CAP)
    acc = np.zeros((g,) + part.shape[1:], F32)
    for i in range(0, n, g):
        blk = part[i:i + g]
        acc[:len(blk)] += blk
    tot = np.zeros(part.shape[1:], F32)
    for b in range(g):
        tot += acc[b]
    return tot


def _dz32(c, d):
    dz = d["dy"] if d.get("dy2") is None else (d["dy"] + d["dy2"]).astype(F32)
    if c.act == 1:                                       # one fma: 1 - y^2 rounded once (float64 holds y^2 exactly)
        dz = (dz * (1.0 - d["y"].astype(F64) ** 2).astype(F32)).astype(F32)
    elif c.act == 2:
        dz = np.where(d["y"] > 0, dz, F32(0)).astype(F32)
    return np.ascontiguousarray(dz, F32)


def emu32(c, d):
    """The quantities of ref64 in float32 (see the module docstring)."""
    if c.entry == "wgrad":
        ac, bc = _chunked(d["a"]), _chunked(d["b"])
        out = {"c": _merge32(np.matmul(ac.transpose(0, 2, 1), bc))}
        if c.bias:
            out["colsum"] = _merge32(ac.sum(1, dtype=F32))
        return out
    if c.entry == "fwd":
        z = d["x"] @ _w_ko(d["w"], c.layout)
        if d["bias"] is not None:
            z = (z + d["bias"]).astype(F32)
        return {"y": _tanh32(z) if c.act == 1 else (np.where(z < 0, F32(0), z) if c.act == 2 else z)}
    dz = _dz32(c, d)
    zc, xc = _chunked(dz), _chunked(d["x"])
    part = np.matmul(zc.transpose(0, 2, 1), xc) if c.layout == 0 else np.matmul(xc.transpose(0, 2, 1), zc)
    out = {"dw": _merge32(part)}
    if c.dx:
        out["dx"] = dz @ np.ascontiguousarray(_w_ko(d["w"], c.layout).T)
    if c.bias:
        out["db"] = _merge32(zc.sum(1, dtype=F32))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# judge
# ------------------------------------------------------------------------------------------------------------------------------
PER_ROW = ("y", "dx")
ACCUMULATED = ("dw", "db", "c", "colsum")


def _t(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a))        # (a copy: the cached arrays are read-only)


def judge(c, ref, got, init=0.0):
    """{quantity: (strict, applied)} for the quantities of `ref` (all of them must be in `got`); init: what the accumulated
    outputs held before the call."""
    m = {}
    for k, r in ref.items():
        r = _t(r).to(torch.float64)
        if init and k in ACCUMULATED:
            r = r + init
        kw = {}
        if k in PER_ROW:
            kw["rows"] = r.shape[0]
        if k == "y" and c.act == 1:                      # the one applied bar that is not the strict one: max(TAU scale, 2e-7) absolute
            floor = torch.full_like(r, TANH_ABS / TAU)
            kw.update(row_terms=floor, tensor_terms=floor)
        m[k] = _metric(_t(got[k]), r, **kw)
    return m


def worst(m, which=1):
    return max((v[which] for v in m.values()), default=0.0)


def passes(m):
    return all(v[1] <= TAU for v in m.values())


# ------------------------------------------------------------------------------------------------------------------------------
# negative controls
# ------------------------------------------------------------------------------------------------------------------------------
CONTROLS = ("last_row", "last_chunk", "last_k_column", "no_dy2", "no_act_derivative", "other_layout", "db_first_chunk")
FULL_RECOMPUTE_MAX_R = 32833          # the controls that need a second full reference are built up to this many rows


PER_ROW_INPUTS = ("x", "dy", "dy2", "y", "a", "b")


def _rows(d, sl):
    return {k: (v[sl] if k in PER_ROW_INPUTS and v is not None else v) for k, v in d.items()}


def _tail_removed(c, d, ref, n):
    """the reference with the last n rows left out: their contribution subtracted from the sums, their rows of y / dx zero"""
    tail = _rows(d, slice(-n, None))
    t = ref64(c, tail)
    out = {}
    for k, r in ref.items():
        if k in PER_ROW:
            out[k] = r.copy()
            out[k][-n:] = 0.0
        else:
            out[k] = r - t[k]
    return out


def controls(c, d=None, ref=None):
    """{control: (wrong answer as a dict of the quantities it changes, coincides)}: coincides = it IS the right answer for this
    case (asserted by the tests, by name).  Built in float64 from the reference and the inputs; nothing wrong is ever run."""
    d = build(c.name) if d is None else d
    ref = reference(c.name) if ref is None else ref
    R = c.R
    out = {"last_row": (_tail_removed(c, d, ref, 1), False)}
    n_last = R - (R - 1) // ROWS * ROWS
    out["last_chunk"] = (_tail_removed(c, d, ref, n_last), False)
    if c.entry == "bwd" and c.bias:
        dz = dz64(c, _rows(d, slice(0, ROWS)))
        out["db_first_chunk"] = ({"db": dz.sum(0)}, R <= ROWS)
    if c.entry != "fwd" and c.K != c.O:
        key = "dw" if c.entry == "bwd" else "c"
        out["other_layout"] = ({key: np.ascontiguousarray(ref[key].T).reshape(ref[key].shape)}, min(c.K, c.O) == 1)   # (a vector has one layout)
    if R > FULL_RECOMPUTE_MAX_R:
        return out
    if c.entry == "fwd" or c.route.startswith("ragged"):
        d2 = dict(d)
        d2["x"] = d["x"].copy()
        d2["x"][:, -1] = 0.0
        out["last_k_column"] = (ref64(c, d2), False)
    if c.entry == "bwd":
        d2 = dict(d)
        d2["dy2"] = None
        out["no_dy2"] = (ref64(c, d2), not c.dy2)
        lin = Case(c[:6] + (0,) + c[7:])
        out["no_act_derivative"] = (ref64(lin, d), c.act == 0)
    return out


def rejected(c, got, wrong, init=0.0):
    """Does judge() fail `got` against the wrong answer (on the quantities the wrong answer has)?"""
    return not passes(judge(c, wrong, got, init))
