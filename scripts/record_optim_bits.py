#!/usr/bin/env python3
"""Record tests/golden/optim_bits.json: the digests of tests/optim_bits.py from the built
extension on the local GPU, with the compiler's version line for the reader.  Run it on
the commit whose bits are to be kept; tests/test_optim_bits_gpu.py compares every later tree
with the file.  usage: record_optim_bits.py [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def hipcc_version():
    try:
        out = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--version"],
                             capture_output=True, text=True, timeout=60).stdout
    except OSError:
        return "unknown"
    lines = [l.strip() for l in out.splitlines() if "version" in l.lower()]
    return lines[0] if lines else "unknown"


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "optim_bits.json"))
    a = ap.parse_args()
    import torch

    import distributed_tensorflow_resnet_amd as dtr
    import optim_bits

    cases = optim_bits.run(dtr.native(required=True), torch.device("cuda:0"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"hipcc": hipcc_version(), "cases": cases}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"{len(cases)} cases, {sum(len(c) for c in cases.values())} digests -> {a.out}")


if __name__ == "__main__":
    main()
