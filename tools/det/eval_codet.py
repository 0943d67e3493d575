#!/usr/bin/env python3
"""tools/det/test_codet.py with the communication flags of upstream's driver:

    python tools/det/eval_codet.py --data /path/V2X-Sim-det/test --com mean --resume ckpt.pth --compress_level 2 --only_v2i 1

--compress_level k (0..8) and --only_v2i 0|1 reach the model's constructor and are checked against the record tools/det/train_codet.py
keeps in its checkpoints; every other flag is test_codet.py's own (v2x_sim_amd/utils/comm.py::run_eval_driver).

    python tools/det/eval_codet.py --data /path/V2X-Sim-det/test --com late --resume lowerbound.pth [--only_v2i 1]

--com late is upstream's late fusion (the table's "Co-lower-bound"): test_codet.py runs as --com lowerbound, the FaFModule it builds exchanges the
agents' detections and suppresses the union per ego (FaFModule.late_fusion; --only_v2i masks the links), and the share of the kept boxes that
came from neighbours is printed after the scores.

    python tools/det/eval_codet.py --data /path/V2X-Sim-det/test --com v2v --resume ckpt.pth --p_com_outage 0.3 --pose_noise 0.5 [--channel_seed 7]

--p_com_outage p (every directed link down with probability p at every step) and --pose_noise sigma (Gaussian noise, metres, on the translation of the
agent-to-agent transforms) are drawn on the device from (--channel_seed, step).  They are an evaluation condition: no checkpoint
records them; --com lowerbound / upperbound / late refuse them, when2com / who2com take --pose_noise only.  The realised share of links up is printed
after the scores.

    python tools/det/eval_codet.py --data /path/V2X-Sim-det/test --com v2v --resume ckpt.pth --map_engine device

--map_engine host | device (default host) travels like every other flag: the driver is tools/det/map_codet.py, which IS test_codet.py for `host` and
scores the same run with one v2x_det_map call for all agents and both thresholds for `device` (same lines, same returned dict)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (ROOT, os.path.join(ROOT, "v2x-sim_amd"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def main(argv=None):
    import map_codet
    from v2x_sim_amd.utils import comm
    return comm.run_eval_driver(map_codet.main, sys.argv[1:] if argv is None else argv)


if __name__ == "__main__":
    main()
