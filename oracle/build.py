"""Build the CPU oracle (TEST INFRASTRUCTURE ONLY) into oracle/_build/liboracle.so.

Strict fp32: no FMA contraction, no fast-math, so the checker is reproducible across hosts.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "gsplat_oracle.c")
OUT_DIR = os.path.join(HERE, "_build")
OUT = os.path.join(OUT_DIR, "liboracle.so")


def build(force: bool = False) -> str:
    os.makedirs(OUT_DIR, exist_ok=True)
    if not force and os.path.exists(OUT) and os.path.getmtime(OUT) >= os.path.getmtime(SRC):
        return OUT
    # processes that start together (the spawned ranks of tests/test_distributed_cpu.py) may all build: each writes its
    # own temporary file, and the rename puts one complete library in place atomically whichever finishes last
    tmp = f"{OUT}.{os.getpid()}.tmp"
    cmd = ["gcc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC",
           "-o", tmp, SRC, "-lm"]
    try:
        subprocess.check_call(cmd)
        os.replace(tmp, OUT)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
