#!/usr/bin/env python3
"""Do two source trees compile to the same device code?  `device_asm_diff.py TREE_A TREE_B [--work DIR]`.

Every file of build.SOURCES is compiled to gfx950 device assembly (build.FLAGS + build.FILE_FLAGS + `--cuda-device-only -S`),
once plain and once with -DDFM_DIAG, in both trees; lines that carry the per-compilation symbol `__hip_cuid_<hash>` are dropped
and the rest compared.  Lists the files that differ and exits non-zero if any do.  Needs hipcc, no GPU.  It only compares:
a refactor that claims "same machine code" runs it against its parent checkout.
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import importlib.util
import os
import subprocess
import sys
import tempfile

FLAVOURS = {"plain": [], "diag": ["-DDFM_DIAG"]}
MAX_JOBS = 16


def load_build(tree: str):
    """The tree's own build.py (its SOURCES / FLAGS / FILE_FLAGS), without importing the package."""
    spec = importlib.util.spec_from_file_location("_dfm_build", os.path.join(tree, "dynamic_factor_models_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def jobs(tree: str, outdir: str) -> dict[tuple[str, str], list[str]]:
    """(source, flavour) -> hipcc command writing outdir/<flavour>/<source>.s"""
    b = load_build(tree)
    out = {}
    for flavour, extra in FLAVOURS.items():
        os.makedirs(os.path.join(outdir, flavour), exist_ok=True)
        for s in b.SOURCES:
            out[(s, flavour)] = [b._hipcc(), *b.FLAGS, *b.FILE_FLAGS.get(s, []), *extra, "--cuda-device-only", "-S",
                                 "-I", os.path.join(tree, "include"), os.path.join(b.CSRC, s),
                                 "-o", os.path.join(outdir, flavour, s.replace(".hip", ".s"))]
    return out


def assemble(cmds: list[list[str]]) -> None:
    with cf.ThreadPoolExecutor(max_workers=min(MAX_JOBS, os.cpu_count() or 2)) as ex:
        for cmd, res in zip(cmds, ex.map(lambda c: subprocess.run(c, capture_output=True, text=True), cmds)):
            if res.returncode:
                sys.exit(f"hipcc failed: {' '.join(cmd)}\n{res.stdout}{res.stderr}")


def stable_lines(path: str) -> list[str]:
    with open(path) as f:
        return [ln for ln in f if "__hip_cuid" not in ln]


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--work", help="keep the assembly files here (default: a temporary directory)")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        work = args.work or tmp
        a = jobs(os.path.abspath(args.tree_a), os.path.join(work, "a"))
        b = jobs(os.path.abspath(args.tree_b), os.path.join(work, "b"))
        assemble(list(a.values()) + list(b.values()))
        differ = [f"{s} [{fl}]" for (s, fl) in b if (s, fl) not in a or stable_lines(a[(s, fl)][-1]) != stable_lines(b[(s, fl)][-1])]
        differ += [f"{s} [{fl}] (only in {args.tree_a})" for (s, fl) in a if (s, fl) not in b]
    print(f"{len(b)} device assemblies compared, {len(differ)} differ")
    for d in differ:
        print("  " + d)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
