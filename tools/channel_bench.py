#!/usr/bin/env python3
"""Cost of degraded links (p_com_outage and pose noise drawn on the device) at 128 frames x 5 agents, none asserted:
  (a) the degrade launch alone (csrc/channel.hip through ops.channel_degrade, V2VNet's plan: rows, link table, pose buffer) in a loop between HIP
      events -- not below the host's issue time of a call;
  (b) the V2VNet forward replayed as ONE hipGraph at p = 0, sigma = 0 (the parent's launches) and at p = 0.3, sigma = 0.5 (one launch more, fresh links
      and noise at every replay): the two graphs alternate inside one process, round by round, and the ratio is taken per round (tools/ab_inproc.sh's rule);
  (c) the host alternative the feature replaces, per step: the mask drawn in Python, set_link_mask, make_plan, the noised poses uploaded, eager launches,
      a synchronise -- on the host clock, alternating with a replay + synchronise of the degraded graph on the same clock.  (The static path cannot
      express a V2VNet ego without a link: the host mask gives such an ego one link back.)
Several rounds each, medians, every round shown.

    python3 tools/channel_bench.py [--frames 128] [--out profiles/channel_bench.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "v2x-sim_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", default=5, type=int)
    ap.add_argument("--frames", default=128, type=int)
    ap.add_argument("--iters", default=5, type=int, help="replays per round and graph")
    ap.add_argument("--rounds", default=7, type=int)
    ap.add_argument("--p", default=0.3, type=float)
    ap.add_argument("--sigma", default=0.5, type=float)
    ap.add_argument("--out", default="", type=str)
    args = ap.parse_args(argv)
    from v2x_sim_amd import ops
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.models.det import V2VNet
    from v2x_sim_amd.utils.synthetic import init_synthetic_weights, synthetic_poses
    if not torch.cuda.is_available():
        raise SystemExit("channel_bench.py measures on the MI355X: no GPU, no figure")
    dev = torch.device("cuda:0")
    A, Bt = args.agents, args.frames
    med = lambda v: float(np.median(v))   # noqa: E731
    lines = ["degraded links at %d frames x %d agents (p_com_outage %g, pose_noise %g m) on %s" % (Bt, A, args.p, args.sigma, torch.cuda.get_device_name(0))]

    model = init_synthetic_weights(V2VNet(Config("train"), num_agent=A), seed=0).to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(1)
    x0 = (torch.rand((A * Bt, 256, 256, 32), generator=g, device=dev) < 0.03).to(torch.bfloat16)
    x0[..., 13:] = 0
    T_host = synthetic_poses(Bt, A, seed=2)
    T = torch.from_numpy(T_host).to(dev)
    nat = torch.full((Bt, A), A)
    plain = model.make_plan(nat, Bt, dev)
    model.set_channel(p_com_outage=args.p, pose_noise=args.sigma, seed=3)
    degraded = model.make_plan(nat, Bt, dev)
    model.set_channel()
    ch = degraded["channel"]

    def events(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / iters            # microseconds per call

    # ---- (a) the launch alone
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    one = lambda: ops.channel_degrade(degraded["items"], A, Bt, ch["coef0"], ch["coef"], None, ch["links"], T, ch["trans"], args.p, args.sigma, 3, step)   # noqa: E731
    events(one, 20)
    t = [events(one, 200) for _ in range(args.rounds)]
    lines.append("(a) degrade launch alone, %d pairs, %d plan rows: median %.1f us per call   rounds: %s" % (
        Bt * A * A, degraded["items"].shape[0], med(t), " ".join("%.1f" % v for v in t)))
    lines.append("    links up at the last step: %d of %d" % (int(ch["links"].sum()), int(ch["possible"])))

    # ---- (b) the forward as one hipGraph, undegraded and degraded, alternating
    graphs = {}
    with torch.no_grad():
        for name, plan in (("plain", plain), ("degraded", degraded)):
            model.forward_nhwc(x0, T, nat, Bt, plan=plan)
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                model.forward_nhwc(x0, T, nat, Bt, plan=plan)
            torch.cuda.current_stream().wait_stream(side)
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                model.forward_nhwc(x0, T, nat, Bt, plan=plan)
            graphs[name].replay()
    torch.cuda.synchronize()
    tp, td = [], []
    for _ in range(args.rounds):
        tp.append(events(graphs["plain"].replay, args.iters) / 1e3)
        td.append(events(graphs["degraded"].replay, args.iters) / 1e3)
    ratios = [d / p for d, p in zip(td, tp)]
    lines.append("(b) V2VNet forward, %d maps, one hipGraph, %d replays per round:" % (A * Bt, args.iters))
    lines.append("    p = 0, sigma = 0:      median %.3f ms   rounds: %s" % (med(tp), " ".join("%.3f" % v for v in tp)))
    lines.append("    p = %g, sigma = %g:  median %.3f ms   rounds: %s" % (args.p, args.sigma, med(td), " ".join("%.3f" % v for v in td)))
    lines.append("    degraded / plain per round: median %.4f   rounds: %s" % (med(ratios), " ".join("%.4f" % v for v in ratios)))
    lines.append("    channel step after the replays: %d" % model.channel_step())

    # ---- (c) the host alternative against a replay of the degraded graph, host clock, alternating
    rng = np.random.default_rng(4)

    def host_step():
        up = rng.random((Bt, A, A)) >= args.p
        for f, i in zip(*np.nonzero(~(up & ~np.eye(A, dtype=bool)).any(2))):
            up[f, i, (i + 1) % A] = True                     # the static rule: no V2VNet ego without a link
        noisy = T_host.copy()
        noisy[..., :3, 3] += (args.sigma * rng.standard_normal((Bt, A, A, 3)) * ~np.eye(A, dtype=bool)[None, :, :, None]).astype(np.float32)
        model.set_link_mask(torch.from_numpy(up))
        plan = model.make_plan(nat, Bt, dev)
        with torch.no_grad():
            model.forward_nhwc(x0, torch.from_numpy(noisy).to(dev), nat, Bt, plan=plan)
        torch.cuda.synchronize()

    def graph_step():
        graphs["degraded"].replay()
        torch.cuda.synchronize()

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        return 1e3 * (time.perf_counter() - t0)
    host_step()
    graph_step()
    th, tg = [], []
    for _ in range(args.rounds):
        th.append(clock(host_step))
        tg.append(clock(graph_step))
    model.set_link_mask(None)
    r = [b / a for a, b in zip(th, tg)]
    lines.append("(c) one step on the host clock (ends in a synchronise):")
    lines.append("    mask in Python + set_link_mask + make_plan + upload + eager launches: median %.3f ms   rounds: %s" % (med(th), " ".join("%.3f" % v for v in th)))
    lines.append("    replay of the degraded graph:                                          median %.3f ms   rounds: %s" % (med(tg), " ".join("%.3f" % v for v in tg)))
    lines.append("    graph / host per round: median %.4f   rounds: %s" % (med(r), " ".join("%.4f" % v for v in r)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
