"""LDS waits of the lean policy tile (the SHAPE 1 rollout builds): no s_waitcnt of the step loop drains a look-ahead
batch that was issued a moment before it.

lgkmcnt is a 4-bit counter on gfx9 and LDS answers in order, so a wait for a value with more than 15 younger LDS reads behind it
cannot be expressed: hipcc clamps it to lgkmcnt(14), and the wave waits for all but the newest 14 reads of the batch it has just
requested.  The tile therefore reads a layer's biases at the front of that layer's OWN fragment batch, takes ONE wait per batch
that the compiler can see (Frags::landed), and requests the first layer's fragments and biases one step ahead, in the env phase.

The measure, on the ISA hipcc emits with the Makefile's flags: simulate the in-order queue over the step loop (every ds_* and every
scalar load is an entry; `s_waitcnt lgkmcnt(n)` pops the oldest until n remain); a popped ds_read_b128 that was issued at most 40
instructions earlier is a YOUNG FORCED READ.  The parent of this change had 67 per step in the two-hop builds (17 at the tile's top,
3 single bias reads behind it, 18 and 4 at the hooks of e1's and e2's middle, 20 at the last hop) and 47 in the one-hop builds (no
last-hop site); recomputed with this helper on that tree.  All five sites were placed, none is left out: what remains are the two
observation reads at the tile's top and the sampler's draw word (3 reads, each consumed right where it is read).

The loop is also walked twice in a row, so that the first-layer request at the END of a step meets the waits at the top of the
next one.  In the ragged builds a wave without an env takes a request of its own in place of the env phase; the listing puts that
block behind the loop's body, a few instructions in front of the back edge, and the walk counts its reads against the waits at the
loop's top (5 / 4 reads): only idle waves run it, the waves with envs never do.  Needs hipcc, no GPU."""
import re

import pytest

from tests import isa

YOUNG = 40
LGKM = re.compile(r"lgkmcnt\((\d+)\)")
PARENT = {2: 67, 1: 47}                  # young forced reads per step before this change, by hop count
DROP = {2: 50, 1: 30}                    # the floor: the sites at the tile's top, the two hooks (and the last hop) are gone

W = "_ZN2cm16rollout_w_kernelILi%dELb1ELb%dELb0ELb1ELi1EEE"            # <LHOPS, PRE, FULLWG, !TAPE, CARRY, SHAPE 1>
WM = "_ZN2cm17rollout_wm_kernelILi%dELb1ELb%dELb1ELi1EEE"             # <LHOPS, PRE, FULLWG, CARRY, SHAPE 1>
PROBE = "_ZN2cm22rollout_w_probe_kernelE"                              # the headline build with the COMMARL_ENV_STOP < 0 clocks


def forced(loop):
    """[(position of the wait, n, outstanding, young forced reads)] for every wait of `loop` that forces a young read."""
    queue, sites = [], []
    for i, ln in enumerate(loop):
        op = ln.split()[0]
        if op.startswith("ds_") or op.startswith("s_load") or op.startswith("s_buffer_load"):
            queue.append((i, op))
        elif op == "s_waitcnt":
            m = LGKM.search(ln)
            if not m:
                continue
            n_pop = max(0, len(queue) - int(m.group(1)))
            popped, queue, out = queue[:n_pop], queue[n_pop:], len(queue)
            young = sum(1 for at, o in popped if o == "ds_read_b128" and i - at <= YOUNG)
            if young:
                sites.append((i, int(m.group(1)), out, young))
    return sites


def _measure(unit, prefix):
    k = isa.kernel(isa.listing(unit), prefix)
    loop = isa.step_loop(k.lines)
    n = isa.counts(loop)
    once = forced(loop)
    twice = [s for s in forced(loop + loop) if s[0] >= len(loop)]       # the second walk: the queue the first one left
    print(prefix, n, "one walk:", once, "second of two walks:", twice)
    assert k.private_segment_fixed_size == 0 and k.vgpr_spill_count == 0
    return n, once, twice


CASES = [("cm_rollout_w", W % (2, 1), 2, True), ("cm_rollout_w", W % (2, 0), 2, False),
         ("cm_rollout_w", W % (1, 1), 1, True), ("cm_rollout_w", W % (1, 0), 1, False),
         ("cm_rollout_w", PROBE, 2, True),
         ("cm_rollout_wm", WM % (2, 1), 2, True), ("cm_rollout_wm", WM % (2, 0), 2, False),
         ("cm_rollout_wm", WM % (1, 1), 1, True), ("cm_rollout_wm", WM % (1, 0), 1, False)]


@pytest.mark.parametrize("unit,prefix,hops,fullwg", CASES, ids=[c[1][8:] for c in CASES])
def test_no_wait_drains_a_young_batch(unit, prefix, hops, fullwg):
    n, once, twice = _measure(unit, prefix)
    assert n["mfma"] >= (288 if hops == 2 else 252), n                  # the loop found is the step: the whole tile is inside
    assert n["ds_read_b128"] >= (167 if hops == 2 else 147), n          # ... with every read of it (the ragged builds: + 24, the idle waves' request)
    total = sum(s[3] for s in once)
    assert max(s[3] for s in once) <= 4, once                           # no single wait forces more than 4 young reads
    assert total <= PARENT[hops] - DROP[hops], once                     # the floor ...
    assert total <= 3 and max(s[3] for s in once) <= 2, once            # ... and what was built: observation reads and draw word
    total2 = sum(s[3] for s in twice)
    assert total2 <= PARENT[hops] - DROP[hops], twice
    assert total2 <= (3 if fullwg else 8), twice                        # across the back edge (ragged: the idle waves' block, see above)
    assert max(s[3] for s in twice) <= (2 if fullwg else 5), twice
