"""Generates tests/golden/g12_sn.npz from the REFERENCE's get_average_dims / get_scaling_params
(train_scaling_based.py), sklearn's DBSCAN and SingleSNSourceDataset / MultiSNSourceDataset (utils/datasets/sn_scaling.py)
on the CPU oracle, through tests/sn_ref.py (build container only: needs the reference and sklearn).

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_sn.py <path of the reference checkout>"""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import sn_ref  # noqa: E402

if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sn_ref.make_g12(sys.argv[1])
