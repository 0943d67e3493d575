#!/usr/bin/env python3
"""Time of one SORT frame for all streams (csrc/track.hip: sort_step_kernel) at the inference step's geometry: 128 streams (5 agents x batch) x 64
detections, 100 consecutive steps -- as 100 eager launches and as one replayed graph of the 100 launches -- and, for comparison, the float64 reference
SORT of tests/track_refs.py on the host for the same input (timed on --host_streams streams x --host_steps steps and scaled: the python reference
takes milliseconds per stream and step).  Nothing here is asserted; the figure to read the result against is the 19.5-20.1 ms inference step the
tracker follows.

    python3 tools/track_bench.py [--streams 128] [--dets 64] [--steps 100] [--out profiles/track_kernel_times.txt]

Scene per stream: `dets` objects on a jittered 8 m grid, constant velocities of up to 0.4 m / frame, 4.5 x 2 m boxes with 0.08 m centre noise and 2 % size
noise, rows shuffled every frame: every track matches every frame (64 x 64 association, mostly the direct reading; a few percent of the frames fall
through to the assignment where neighbours overlap)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "v2x-sim_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def make_input(streams, dets, steps, seed=0):
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(dets)))
    grid = np.stack(np.meshgrid(np.arange(side), np.arange(side)), -1).reshape(-1, 2)[:dets] * 8.0
    pos = grid[None] + rng.uniform(-1.5, 1.5, (streams, dets, 2))
    vel = rng.uniform(-0.4, 0.4, (streams, dets, 2))
    size = np.array([4.5, 2.0])
    out = np.zeros((steps, streams, 64, 4), np.float32)
    for f in range(steps):
        c = pos + vel * f + rng.normal(0, 0.08, pos.shape)
        sz = size * (1 + 0.02 * rng.normal(0, 1, pos.shape))
        b = np.concatenate([c - sz / 2, c + sz / 2], -1)
        for s in range(streams):
            out[f, s, :dets] = b[s, rng.permutation(dets)]
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default=128, type=int)
    ap.add_argument("--dets", default=64, type=int)
    ap.add_argument("--steps", default=100, type=int)
    ap.add_argument("--rounds", default=5, type=int)
    ap.add_argument("--direct", default=1, type=int)
    ap.add_argument("--host_streams", default=2, type=int)
    ap.add_argument("--host_steps", default=20, type=int)
    ap.add_argument("--out", default="", type=str)
    args = ap.parse_args(argv)
    from v2x_sim_amd import ops
    dev = torch.device("cuda:0")
    n, steps = args.streams, args.steps
    host_in = make_input(n, args.dets, steps)
    det = torch.from_numpy(host_in).to(dev)
    cnt = torch.full((n,), args.dets, dtype=torch.int32, device=dev)
    st = (torch.zeros((n, 64, 17), device=dev), torch.zeros((n, 64, 5), dtype=torch.int32, device=dev), torch.zeros((n, 4), dtype=torch.int32, device=dev))
    out = (torch.zeros((n, 64, 4), device=dev), torch.zeros((n, 64), dtype=torch.int32, device=dev), torch.zeros((n, 64), dtype=torch.int32, device=dev),
           torch.zeros((n,), dtype=torch.int32, device=dev))

    def run():
        for f in range(steps):
            ops.sort_step(det[f], cnt, *st, out=out, direct=bool(args.direct))

    def timed(fn):
        for t in st:
            t.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    timed(run)
    eager = [timed(run) for _ in range(args.rounds)]
    reported = int(out[3].sum())
    tracks = int(st[2][:, 0].sum())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    timed(g.replay)
    graph = [timed(g.replay) for _ in range(args.rounds)]

    import track_refs as R
    hs, hf = min(args.host_streams, n), min(args.host_steps, steps)
    t0 = time.perf_counter()
    for s in range(hs):
        ref = R.SortRef(direct=bool(args.direct))
        for f in range(hf):
            ref.step(host_in[f, s, :args.dets])
    host = (time.perf_counter() - t0) / (hs * hf)

    e, gr = float(np.median(eager)), float(np.median(graph))
    lines = ["sort_step_kernel: %d streams x %d detections, %d steps, direct = %d; medians of %d rounds on %s" % (n, args.dets, steps, args.direct, args.rounds,
                                                                                                          torch.cuda.get_device_name(0)),
             "after the last step: %d live tracks, %d reported" % (tracks, reported),
             "eager launches : %8.3f ms per %d steps = %7.1f us per step" % (e, steps, 1e3 * e / steps),
             "one graph      : %8.3f ms per %d steps = %7.1f us per step" % (gr, steps, 1e3 * gr / steps),
             "host reference : %8.3f ms per stream and step (float64 python, %d streams x %d steps) = %.0f ms per step of %d streams (scaled)"
             % (1e3 * host, hs, hf, 1e3 * host * n, n),
             "for scale: the inference step this follows takes 19.5-20.1 ms for the same 128 maps"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
