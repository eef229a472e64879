#!/usr/bin/env python3
"""Regenerate profiles/r12_splat_loss_accuracy.txt: run tests/test_gpu_splat_loss.py on the GPU and keep the "loss-accuracy"
line of every comparison (its largest error / bound ratio; the bounds are derived in tests/splat_loss_reference.py).
The file is written only when every test passes.  python tools/splat_loss_accuracy.py [--out FILE]"""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_splat_loss_accuracy.txt"))
    args = ap.parse_args(argv)
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_splat_loss.py"), "-m", "gpu", "-q",
                        "-s", "-p", "no:cacheprovider"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    sys.stdout.write(p.stdout[-3000:])
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-2000:])
        return p.returncode
    lines = re.findall(r"loss-accuracy.*", p.stdout)
    tail = p.stdout.strip().splitlines()[-1]
    with open(args.out, "w") as f:
        f.write("# python tools/splat_loss_accuracy.py on an MI355X: tests/test_gpu_splat_loss.py, the largest error / bound ratio of\n"
                "# every comparison (bounds: tests/splat_loss_reference.py); pytest: " + tail.strip("= ") + "\n")
        f.write("\n".join(lines) + "\n")
    print(f"{len(lines)} lines -> {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
