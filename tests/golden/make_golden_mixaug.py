"""Generates tests/golden/g16_mixaug.npz from the REFERENCE's CosMixSourceDataset.merge_data with an augmentation list
and Mix3DSourceDataset.merge_data (utils/datasets/cosmix.py, mix3D.py, utils/common/augmentation.py) on the CPU oracle,
through tests/mixaug_ref.py (build container only: needs the reference and scipy).

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_mixaug.py <path of the reference checkout>"""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import mixaug_ref  # noqa: E402

if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    mixaug_ref.make_g16(sys.argv[1])
