"""Was a split of one Python module into several a pure move?  Compares every top-level def / class / assignment of OLD at a git
revision with the same-named node of the NEW files by ast.dump (comments and layout do not count, docstrings do), and lists what
differs, what is missing and what is new.

  python tools/movecheck.py HEAD~1 com-marl_amd/nets.py com-marl_amd/nets/*.py"""
import ast
import subprocess
import sys


def nodes(src):
    """{name: dump} of the top-level definitions; an assignment is listed under each plain name it binds."""
    out = {}
    for n in ast.parse(src).body:
        if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
            out[n.name] = ast.dump(n)
        elif isinstance(n, (ast.Assign, ast.AnnAssign, ast.AugAssign)):
            for t in n.targets if isinstance(n, ast.Assign) else [n.target]:
                for e in (t.elts if isinstance(t, (ast.Tuple, ast.List)) else [t]):
                    if isinstance(e, ast.Name):                 # (an attribute or subscript target binds no module-level name)
                        out[e.id] = ast.dump(n)
    return out


def main(rev, old, new):
    was = nodes(subprocess.check_output(["git", "show", f"{rev}:{old}"], text=True))
    now = {}
    for path in new:
        for name, dump in nodes(open(path).read()).items():
            if name in now:
                print(f"defined twice: {name} ({path})")
            now[name] = dump
    same = [n for n in was if now.get(n) == was[n]]
    print(f"{len(same)} of {len(was)} definitions of {rev}:{old} are unchanged in {len(new)} files")
    for n in was:
        if n not in now:
            print(f"missing: {n}")
        elif now[n] != was[n]:
            print(f"differs: {n}")
    for n in now:
        if n not in was:
            print(f"new: {n}")
    return 0 if len(same) == len(was) and len(now) == len(was) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2], sys.argv[3:]))
