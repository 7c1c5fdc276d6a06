"""Generates tests/golden/g15_scans.npz from the REFERENCE's file datasets (utils/datasets/semantickitti.py, nuscenes.py,
synth4d.py: listing, LUT construction, load_label_kitti / load_label_nusc, the cached `data` dict of __getitem__, the
validation-phase item, get_dataset_stats) over the tiny file trees of tests/scans_ref.py, on the CPU oracle's
sparse_quantize (build container only: needs the reference, PyYAML and tqdm).

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_scans.py <path of the reference checkout>"""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import scans_ref  # noqa: E402

if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    scans_ref.make_g15(sys.argv[1])
