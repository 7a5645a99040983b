"""Records g25_ap_host_ref.npz: this project's OWN host eval_class output (stats_device="cpu") on the adversarial split of
tests/ap_split.py and on fixture g10's annotations, for the three overlap kinds and both difficulty rules, the rotated kinds under
the CPU oracle of the IoU kernel (oracle.ext_cpu.patch_package).  It was run on commit 9118037, the last one whose host path
built a _Split per (class, difficulty, overlap kind); tests/test_kitti_ap_table.py::test_host_eval_class_is_what_it_was holds the
host path on the shared table to these bits.  Run on a later tree it would record the code under test, so it refuses to.

  python tests/golden/make_golden_ap_host.py          (in a checkout of 9118037 with this file copied in; CPU, built library, oracle)"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import ap_split                                                                        # noqa: E402
from oracle import ext_cpu                                                             # noqa: E402

KE = importlib.import_module("3d_adapt_auto_driving_amd.kitti_eval")
LEVELS = np.array([[[0.7, 0.5, 0.5]] * 3, [[0.7, 0.5, 0.5], [0.5, 0.25, 0.25], [0.5, 0.25, 0.25]]])       # [level, kind, class]
RULES = (("new", "kitti", [0, 1, 2, 3, 4, 5]), ("old", "waymo", [0, 1, 2]))


def splits():
    gl, dl = ap_split.make_split(0)
    yield "helper", ap_split.as_annos(KE, gl), ap_split.as_annos(KE, dl)
    z = np.load(os.path.join(HERE, "g10_ap_eval_ref.npz"))
    yield "g10", [KE.annos_from_lines(str(s).split("\n")) for s in z["gt_lines"]], [KE.annos_from_lines(str(s).split("\n")) for s in z["dt_lines"]]


def curves(gt, dt, rule, dataset, diffs, kind):
    """(3, n_class, n_diff, n_lev, 41): precision, recall, orientation"""
    with ext_cpu.patch_package():
        r = KE.eval_class(gt, dt, [0, 1, 2], dataset, diffs, kind, LEVELS, compute_aos=(kind == 0), difficulty_metric=rule)
    return np.stack([r["precision"], r["recall"], r["orientation"]], 0)


if __name__ == "__main__":
    if hasattr(KE, "HostStats"):
        sys.exit("this tree's host path already runs on the split table: record from commit 9118037 (see the docstring)")
    out = {"%s_%s_%d" % (name, rule, kind): curves(gt, dt, rule, dataset, diffs, kind)
           for name, gt, dt in splits() for rule, dataset, diffs in RULES for kind in (0, 1, 2)}
    np.savez_compressed(os.path.join(HERE, "g25_ap_host_ref.npz"), **out)
    print({k: (v.shape, int(np.count_nonzero(v))) for k, v in out.items()})
