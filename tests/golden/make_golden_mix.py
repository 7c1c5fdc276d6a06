"""Generates tests/golden/g11_mix.npz from the REFERENCE's PointCutMixSourceDataset.merge_data and
CoSMixSourceDataset.merge_data (utils/datasets/pointcutmix.py, utils/datasets/cosmix.py) on the CPU oracle, through
tests/mix_ref.py (build container only: needs the reference).

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_mix.py <path of the reference checkout>"""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import mix_ref  # noqa: E402

if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    mix_ref.make_g11(sys.argv[1])
