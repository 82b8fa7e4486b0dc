"""Regenerates tests/golden/matgen/*.txt.gz: the files the reference's own matrix_generator.cpp writes for the argument
lists the tests use (tests/test_oracle.py, tests/test_harness.py), gzip-compressed byte for byte.

The tests compare against these stored outputs, so they run wherever the repository is checked out.  Regenerating needs
the reference generator binary oracle/_ref/matgen (built by `make -C oracle ref` when the reference tree is present).
Run from the repo root:  python tests/golden/make_golden_matgen.py
"""
import gzip
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "matgen")
REF_MATGEN = os.path.join(ROOT, "oracle", "_ref", "matgen")

ARGS = [("128", "2", "exp"), ("64", "2", "exp"), ("40", "7", "lin", "0.3"), ("33", "31", "lin"), ("30", "3", "lin"),
        ("20", "5", "exp", "0.5")]


def golden_path(args):
    return os.path.join(OUT, "matgen_" + "_".join(args) + ".txt.gz")


def main():
    if not os.path.exists(REF_MATGEN):
        sys.exit(f"{REF_MATGEN} is missing: build it with `make -C oracle ref` from a tree that has the reference")
    os.makedirs(OUT, exist_ok=True)
    with tempfile.TemporaryDirectory() as td:
        for args in ARGS:
            f = os.path.join(td, "m.txt")
            subprocess.run([REF_MATGEN, f, *args], check=True, capture_output=True)
            with open(f, "rb") as src, open(golden_path(args), "wb") as dst:
                dst.write(gzip.compress(src.read(), compresslevel=9, mtime=0))
            print(golden_path(args))


if __name__ == "__main__":
    main()
