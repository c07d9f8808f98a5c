#!/usr/bin/env python
"""Record tests/golden/stack_launches.json: the launch names and result hashes tests/test_gpu_stack_frame.py pins.

Run on the MI355X at the commit whose behaviour is to be kept (the parent of a refactor of the propagation stacks):

    python tools/gen_stack_launch_golden.py [--out tests/golden/stack_launches.json]

Every case of test_gpu_stack_frame.CASES runs twice.  The launch lists, routes and callback orders of the two runs must agree; a tensor
whose bytes differ between them is recorded as "unstable".  More than one unstable tensor in ten is an error: fix the case, not the cap."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import test_gpu_stack_frame as sf
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=sf.FIXTURE)
    args = ap.parse_args()
    fixture, n, n_unstable = {}, 0, 0
    for name in sorted(sf.CASES):
        a, b = sf.run_case(name), sf.run_case(name)
        for key in ("fwd", "bwd", "routes", "grad_ready", "refused"):
            assert a.get(key) == b.get(key), (name, key, a.get(key), b.get(key))
        assert sorted(a["tensors"]) == sorted(b["tensors"]), name
        for k, v in a["tensors"].items():
            n += 1
            if b["tensors"][k] != v:
                a["tensors"][k] = sf.UNSTABLE
                n_unstable += 1
                print(f"unstable: {name} {k}")
        fixture[name] = a
        print(f"{name}: {len(a['fwd'])} forward / {len(a['bwd'])} backward launches, {len(a['tensors'])} tensors", flush=True)
    assert n_unstable <= sf.UNSTABLE_CAP * n, f"{n_unstable} of {n} tensors are unstable"
    with open(args.out, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(fixture[k], sort_keys=True)}" for k in sorted(fixture)) + "\n}\n")   # one case per line
    print(f"wrote {args.out}: {len(fixture)} cases, {n} tensors, {n_unstable} unstable")


if __name__ == "__main__":
    main()
