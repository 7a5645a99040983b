"""Child process of tests/test_eval_transforms.py: the evaluator's command line (kitti_eval.main) with the rotated IoU served by the CPU
oracle, so that it runs without a GPU.  argv: the command line's own arguments.  Not a test module."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ext_cpu  # noqa: E402
from oracle import oracle as O  # noqa: E402

O.build()
KE = importlib.import_module("3d_adapt_auto_driving_amd.kitti_eval")
with ext_cpu.patch_package():
    KE.main(sys.argv[1:])
