"""Generates tests/golden/g10_minkunet34robust.npz from the REFERENCE's MinkUNet34Robust
(utils/models/minkunet_robustnet.py) and IWLoss (utils/losses/losses.py) on the CPU oracle, with the instance norm of
tests/ibn_ref.py and the in-place ReLU of tests/robust_ref.py (build container only: needs the reference).

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_robust.py <path of the reference checkout>"""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import robust_ref  # noqa: E402

if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    robust_ref.make_g10(sys.argv[1])
