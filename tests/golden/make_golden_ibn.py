"""Generates tests/golden/g9_minkunet34ibn.npz from the REFERENCE's MinkUNet34IBN (utils/models/minkunet_ibn.py) on
the CPU oracle plus the instance-norm restatement of tests/ibn_ref.py (build container only: needs the reference).

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_ibn.py

Pins the IBN wiring to the reference class, not ME's instance norm (see tests/ibn_ref.py)."""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ibn_ref  # noqa: E402

if __name__ == "__main__":
    ibn_ref.make_g9(*sys.argv[1:2])
