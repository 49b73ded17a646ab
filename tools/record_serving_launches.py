#!/usr/bin/env python3
"""Records tests/golden/serving_launches.json: per serving case (tests/serving_cases.py) the timing hook's (role, kernel, launches) list and a
SHA-256 of every returned tensor's bytes.  Run it ONCE at the commit a refactor starts from; tests/test_gpu_serving_launches.py then replays the
cases on the refactored tree and asserts equality -- same kernels, same counts, same bits.

Every case runs twice.  A case whose hashes differ between the two runs is recorded with its launch list only (the test then compares that alone)
and named under "unstable" and on stdout.

    python tools/record_serving_launches.py [--out tests/golden/serving_launches.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import serving_cases as SC  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "serving_launches.json"))
    args = ap.parse_args()
    # (many cases launch the same list, and the lists the same kernels: each distinct (role, kernel) and each distinct list is written once, by index)
    cases, kernels, lists, unstable = {}, [], [], []
    for hm, setting in SC.GROUPS:
        first, second = SC.run_group(hm, setting), SC.run_group(hm, setting)
        for cid, (launches, hashes) in first.items():
            again_launches, again_hashes = second[cid]
            if launches != again_launches:
                raise SystemExit(f"{cid}: the launch list itself differs between two runs:\n{launches}\n{again_launches}")
            for role, kernel, _ in launches:
                if [role, kernel] not in kernels:
                    kernels.append([role, kernel])
            packed = [[kernels.index([role, kernel]), n] for role, kernel, n in launches]
            if packed not in lists:
                lists.append(packed)
            cases[cid] = {"launches": lists.index(packed)}
            if hashes == again_hashes:
                cases[cid]["sha256"] = hashes
            else:
                unstable.append(cid)
        print(f"{SC.group_id(hm, setting)}: {len(first)} cases", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"batch": SC.B, "hm_chunk": SC.CHUNK, "kernels": kernels, "launch_lists": lists, "cases": cases, "unstable": unstable}, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(f"{len(cases)} cases, {len(lists)} distinct launch lists -> {args.out}; unstable (launch list only): {unstable or 'none'}")


if __name__ == "__main__":
    main()
