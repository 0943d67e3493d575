#!/usr/bin/env python3
"""tools/seg/test_seg.py with the communication flags: --compress_level k (0..8) and --only_v2i 0|1 reach V2VNetSeg's constructor and are
checked against the record tools/seg/train_seg.py keeps in its checkpoints; every other flag is test_seg.py's own
(v2x_sim_amd/utils/comm.py::run_eval_driver)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (ROOT, os.path.join(ROOT, "v2x-sim_amd"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def main(argv=None):
    import test_seg
    from v2x_sim_amd.utils import comm
    return comm.run_eval_driver(test_seg.main, sys.argv[1:] if argv is None else argv)


if __name__ == "__main__":
    main()
