"""Generates tests/golden/g13_augment.npz from the REFERENCE's RandomRotation / RandomScale
(utils/common/augmentation.py), random_sample (utils/datasets/dataset.py), filter_bounds and getBEVImageNew
(utils/datasets/semantickitti_bev.py) on the CPU oracle's sparse_quantize, through tests/augment_ref.py (build container
only: needs the reference and scipy).

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_augment.py <path of the reference checkout>"""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import augment_ref  # noqa: E402

if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    augment_ref.make_g13(sys.argv[1])
