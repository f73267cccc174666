#!/usr/bin/env python3
"""Write tests/golden/adamw_bits.json: the digests tests/test_gpu_adamw_bits.py compares against, from that module's own case list
and the library this process loads (csrc/libdosx.so, or DOSX_LIB).  Run it on the commit whose bits are to be pinned - before a
change to the optimizer's kernels, not after - on an MI355X.

The file names the commit (``git rev-parse HEAD`` of this tree, or --commit where the tree has no .git).  An existing fixture
is not overwritten without --force.

usage: python tools/record_adamw_bits.py [--out PATH] [--commit SHA] [--force]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import test_gpu_adamw_bits as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=T.FIXTURE)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--force", action="store_true")
    args = ap.parse_args()
    if os.path.exists(args.out) and not args.force:
        raise SystemExit(f"{args.out} exists: the recorded bits are the reference, --force replaces them")
    commit = args.commit or subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, check=True, capture_output=True,
                                           text=True).stdout.strip()
    if len(commit) != 40:
        raise SystemExit(f"--commit wants the full 40-digit hash, got {commit!r}")
    cases = {}
    for c in T.CASES:
        cases[c["id"]] = T.run_case(c)
        print(c["id"], cases[c["id"]]["p"][:16], cases[c["id"]]["m"][:16], cases[c["id"]]["v"][:16])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"commit": commit, "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(cases)} cases -> {args.out} (library of {commit})")


if __name__ == "__main__":
    main()
