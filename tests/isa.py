"""The one place tests get gfx950 ISA from: the listing of a translation unit of libcommarl_hip.so, compiled with the command
csrc/Makefile itself builds that unit with (its target-specific flags included), and the parsing the static guards share.
Needs hipcc, no GPU.

    python -m tests.isa diff <other-tree>

compiles every unit of the Makefile's SRC in this tree and in <other-tree> (each with its own Makefile's command) and reports
per kernel symbol whether the instruction streams and the resource footprints (registers, LDS, scratch, spills) are the same,
also for a symbol the other tree has in another unit ("moved from"); the exit status is non-zero if any differ or are missing."""
import functools
from concurrent.futures import ThreadPoolExecutor
import os
import re
import shlex
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MFMA = re.compile(r"^v_mfma_")
# what issues on the vector ALU: v_* without the matrix pipe; the AGPR copies are VALU instructions as well
VALU = re.compile(r"^v_(?!mfma_)")
FLAT_OR_SCRATCH = re.compile(r"^(flat_(load|store|atomic)|scratch_)")
FOOTPRINT_KEYS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count",
                  "sgpr_spill_count")


def csrc(root=ROOT):
    return os.path.join(root, "com-marl_amd", "csrc")


def compile_command(unit, out, root=ROOT):
    """The Makefile's own hipcc command for _build/<unit>.o, with `-c <src> -o <obj>` swapped for a device-only listing to `out`."""
    dry = subprocess.run(["make", "-C", csrc(root), "-n", "-B", "--no-print-directory", f"_build/{unit}.o"],
                         check=True, capture_output=True, text=True).stdout
    cmds = [shlex.split(ln) for ln in dry.splitlines() if f"{unit}.hip" in ln and " -c " in ln]
    assert len(cmds) == 1, f"expected one compile line for {unit}.hip from the Makefile, got:\n{dry}"
    cmd = cmds[0]
    i, o = cmd.index("-c"), cmd.index("-o")
    assert o == i + 2 and o + 2 == len(cmd), f"unexpected shape of the Makefile's compile line: {cmd}"
    return cmd[:i] + ["-S", "--cuda-device-only", "-w", "-o", str(out), cmd[i + 1]]


@functools.lru_cache(maxsize=None)
def _listing(unit, root):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, unit + ".s")
        cmd = compile_command(unit, out, root)
        if not (shutil.which(cmd[0]) or os.path.exists(cmd[0])):
            return None
        subprocess.check_call(cmd, cwd=csrc(root))
        return open(out).read()


def listing(unit, root=ROOT):
    """The gfx950 ISA listing of csrc/<unit>.hip; compiled once per unit and process.  Skips the calling test without hipcc."""
    asm = _listing(unit, root)
    if asm is None:
        import pytest
        pytest.skip("hipcc not available")
    return asm


class Kernel:
    """One kernel of a listing: mangled name, its metadata block and its instruction lines (labels kept, comments and
    directives dropped)."""

    def __init__(self, name, meta, lines):
        self.name, self.meta, self.lines = name, meta, lines

    def _meta_int(self, key):
        return int(re.search(r"\." + key + r":\s+(\d+)", self.meta).group(1))

    @property
    def private_segment_fixed_size(self):
        return self._meta_int("private_segment_fixed_size")

    @property
    def vgpr_spill_count(self):
        return self._meta_int("vgpr_spill_count")

    @property
    def footprint(self):
        """What decides occupancy: register, LDS, scratch and spill counts.  (kernels() splits the listing at `.agpr_count:`,
        so that one value is what the block opens with.)"""
        fp = {key: self._meta_int(key) for key in FOOTPRINT_KEYS}
        fp["agpr_count"] = int(re.match(r"\s*(\d+)", self.meta).group(1))
        return fp

    def count(self, prefix):
        return sum(1 for ln in self.lines if ln.startswith(prefix))

    @property
    def has_flat_or_scratch(self):
        return any(FLAT_OR_SCRATCH.match(ln) for ln in self.lines)

    @property
    def barriers(self):
        return self.count("s_barrier")


def _instruction_lines(body):
    lines = []
    for ln in body.splitlines():
        ln = ln.split(";")[0].strip()
        if ln and (not ln.startswith(".") or re.match(r"\.LBB\d+_\d+:", ln)):
            lines.append(ln)
    return lines


def kernels(asm, name_part=""):
    """Every kernel of the listing whose mangled name contains `name_part`.  A kernel is what has a metadata block; each must
    also have a body in the text (the label line carries a trailing "; @name" comment)."""
    found = []
    for meta in re.split(r"\n\s+- \.agpr_count:", asm)[1:]:                 # one metadata block per kernel
        name = re.search(r"\.name:\s+(\S+)", meta).group(1)
        if name_part not in name:
            continue
        body = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)\n\.Lfunc_end", asm, re.M | re.S)
        assert body, "no body in the listing for " + name
        found.append(Kernel(name, meta, _instruction_lines(body.group(1))))
    return found


def kernel(asm, prefix):
    """The one kernel whose mangled name starts with `prefix`."""
    ks = [k for k in kernels(asm) if k.name.startswith(prefix)]
    assert len(ks) == 1, f"expected one kernel {prefix}*, found {[k.name for k in ks]}"
    return ks[0]


def step_loop(lines):
    """The largest span closed by a backward branch: the step loop (everything else in the body is straight-line set-up, the
    staging rounds and the short element loops of the env phase)."""
    label_at = {ln[:-1]: i for i, ln in enumerate(lines) if ln.endswith(":")}
    best = None
    for i, ln in enumerate(lines):
        m = re.match(r"s_c?branch\S*\s+(\.LBB\d+_\d+)$", ln)
        if m and m.group(1) in label_at and label_at[m.group(1)] < i:
            if best is None or i - label_at[m.group(1)] > best[1] - best[0]:
                best = (label_at[m.group(1)], i)
    assert best is not None, "no backward branch in the kernel body: the step loop was not found"
    loop = [ln for ln in lines[best[0]:best[1] + 1] if not ln.endswith(":")]
    return loop


def counts(loop):
    mfma = [ln for ln in loop if MFMA.match(ln)]
    return {
        "insts": len(loop),
        "mfma": len(mfma),
        # an A / B source operand in AGPRs: `v_mfma_... v[0:3], a[8:11], v[..], v[..]` (operands 2 and 3)
        "mfma_agpr_src": sum(1 for ln in mfma if any(op.strip().startswith("a[") for op in ln.split(None, 1)[1].split(", ")[1:3])),
        "accvgpr_read": sum(1 for ln in loop if ln.startswith("v_accvgpr_read_b32")),
        "accvgpr_write": sum(1 for ln in loop if ln.startswith("v_accvgpr_write_b32")),
        "valu": sum(1 for ln in loop if VALU.match(ln)),
        "cvt_f32_f16": sum(1 for ln in loop if ln.startswith("v_cvt_f32_f16")),
        "readlane": sum(1 for ln in loop if ln.startswith("v_readlane_b32")),
        "s_nop": sum(1 for ln in loop if ln.startswith("s_nop")),
        "salu": sum(1 for ln in loop if ln.startswith("s_")),
        "ds_read_b128": sum(1 for ln in loop if ln.startswith("ds_read_b128")),
    }


def units(root=ROOT):
    """The translation units of the library: the Makefile's SRC."""
    src = re.search(r"^SRC\s*:=\s*(.*)$", open(os.path.join(csrc(root), "Makefile")).read(), re.M).group(1)
    return [s[:-len(".hip")] for s in src.split()]


def _streams(unit, root):
    asm = _listing(unit, root)
    if asm is None:
        sys.exit("hipcc not available")
    # not part of an instruction: the compilation-unit id (a hash of the source text) and the function's ordinal in its
    # unit's block labels (.LBB<ordinal>_<block>: the order in which the host code first names the instantiations)
    def norm(ln):
        return re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"__hip_cuid_\w+", "__hip_cuid", ln))
    return {k.name: ([norm(ln) for ln in k.lines], k.footprint) for k in kernels(asm)}


def diff(other):
    """Per kernel symbol of every unit of either tree: identical / differs / only here / only there, where identical covers the
    instruction stream and the resource footprint.  A symbol the other tree has in a different unit is compared all the same
    and reported as moved.  Returns the number that are not identical."""
    here, there = units(ROOT), units(other)
    with ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as pool:           # the compiles, side by side; _listing keeps them
        list(pool.map(lambda job: _listing(*job), [(u, ROOT) for u in here] + [(u, other) for u in there]))
    a = {(u, name): k for u in here for name, k in _streams(u, ROOT).items()}
    b = {(u, name): k for u in there for name, k in _streams(u, other).items()}
    elsewhere = {}                                # symbol -> the other tree's units that hold it and have no such symbol here
    for u, name in sorted(b):
        if (u, name) not in a:
            elsewhere.setdefault(name, []).append(u)
    bad = 0
    for u, name in sorted(a):
        src = u if (u, name) in b else elsewhere[name].pop(0) if elsewhere.get(name) else None
        if src is None:
            verdict = "only here"
        else:
            verdict = "identical" if a[u, name] == b[src, name] else "differs"
            verdict += f" (moved from {src})" if src != u else ""
        bad += not verdict.startswith("identical")
        print(f"{u}: {verdict:10s} {name}" + (f" ({len(a[u, name][0])} instruction lines)" if verdict.startswith("identical") else ""))
    gone = [(u, name) for name, us in sorted(elsewhere.items()) for u in us]
    for u, name in gone:
        print(f"{u}: {'only there':10s} {name}")
    bad += len(gone)
    print(f"{len(a) + len(gone)} kernels in {len(set(here) | set(there))} units, {bad} not identical")
    return bad


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "diff" or not os.path.isdir(sys.argv[2]):
        sys.exit(__doc__)
    sys.exit(1 if diff(os.path.abspath(sys.argv[2])) else 0)
