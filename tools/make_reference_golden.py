#!/usr/bin/env python3
"""Record the reference implementation's results for the seeded cases of
tests/reference_cases.py under tests/golden/reference_parity/.

    python tools/make_reference_golden.py --reference /path/to/RAFT-NCUP/core

The reference is only imported and run (CPU, fp32); nothing of it is copied.
Needed again only when a case in tests/reference_cases.py changes.
"""

import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import reference_cases as rc  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "reference_parity")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True,
                    help="the reference checkout's core/ directory")
    ap.add_argument("--only", nargs="*", default=None)
    cli = ap.parse_args()
    ref = rc.Reference(os.path.abspath(cli.reference))
    os.makedirs(OUT, exist_ok=True)

    for name in rc.ARRAY_CASES:
        if cli.only and name not in cli.only:
            continue
        arrays = rc.run_arrays(name, ref)
        path = os.path.join(OUT, name + ".npz")
        np.savez(path, **arrays)
        print("%-32s %4d arrays %8d bytes" % (name, len(arrays),
                                              os.path.getsize(path)))

    if not cli.only:
        surfaces = {name: rc.run_json(name, ref) for name in rc.JSON_CASES}
        with open(os.path.join(OUT, "surfaces.json"), "w") as f:
            json.dump(surfaces, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
