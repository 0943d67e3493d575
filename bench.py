#!/usr/bin/env python3
"""Headline benchmark: BEV frames/sec of V2VNet 5-agent detection on MI355X (BASELINE.json metric).

  python bench.py --gpus N --steps K --warmup W
      N > 1 without a launcher environment: this process starts `python -m torch.distributed.run --nproc-per-node N`
      on itself BEFORE any GPU call and relays rank 0's JSON line and the exit code; under torchrun (WORLD_SIZE set)
      it is a rank.  `--dry-run` walks launcher + rendezvous + shard plan + collective on gloo without a GPU.

One step = one pass of the whole hot path over one batch of synthetic frames, inputs already
resident in HBM:  LiDAR points -> voxel scatter (a1) -> encoder (a2) -> [RCCL all-gather of the
fusion-layer maps when N > 1] -> warp + ConvGRU (a3, a4) -> decoder (a6) -> det heads (a7).
Work items are (agent, frame) maps sharded agent-major over the ranks (v2x_sim_amd/parallel.py);
per-GPU work is fixed as N grows (weak scaling): frames = frames_per_gpu * N, run as two half-batches whose
all-gathers are asynchronous and hidden under the other half's compute.

Execution mode is the SAME for every N (`exec_mode` in the record): the step's four collective-free segments
(encoder A, encoder B, fusion+decoder+heads A, ... B) are replayed from hipGraphs and the exchange runs between them
(at N = 1 there is nothing to exchange), so the 1 -> 8 curve compares equals.  The two half-batches run on two streams
(own graph memory pools) and are joined at the end of the step: one half's kernels fill the tails and the HBM-bound
phases of the other (+2.3...3.0 % at N = 1 against `--graph 4`, the one-stream order).

Prints ONE JSON line (rank 0).  A plain run does what the headline needs and nothing else: set-up, warm-up, the K timed steps,
`--dump-outputs`, the line.  `--full` adds everything else the benchmark measures or checks, after the timed region and in runs of
their own: `roofline` is computed from HIP events recorded live around every kernel launch of an instrumented pass on the launch
stream; `cpu_baseline` times the CPU oracle (oracle/, PyTorch-CPU fp32) on a bounded sample of the same workload; parse() lists the rest.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "v2x-sim_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

# MI355X peaks (/opt/skills/guides/MI355X_MICROARCH.md): HBM3E 8.0 TB/s spec, bf16 MFMA ~2.5 PF dense
# rocprofv3 FETCH_SIZE -> bytes.  The guide's gfx950 correction (x 2: wide coalesced reads are tallied at half their bytes) was CALIBRATED in round 6 on this library's own access
# patterns, as the guide prescribes for anything but wide reads (profiles/r06_fetch_calibration.txt: tools/fetch_calib_probe.hip, tools/r06/run9.sh): 1-KiB-per-instruction reads
# x 2.00, 64-byte segment reads (the 32-channel patch chunks of the streamed kernels) x 1.0-1.1.  The ConvGRU kernel's raw count splits 54 % patch segments / 46 % weight pieces
# (phase-removal builds) -> x 1.52.  Kernels without an entry keep the guide's x 2 (`fetch_factor_calibrated` in the record says which it was).
FETCH_FACTOR_DEFAULT = 2.0
FETCH_FACTOR = {"conv3x3_stream8g_kernel<96, 2, false>": (168.6 * 1.10 + 142.2 * 2.0) / 309.6}
PEAK_HBM_GBS = 8000.0
PEAK_MFMA_TFLOPS = 2500.0
AGENTS = 5
POINTS_PER_SWEEP = 65536
# committed PMC traffic summaries, newest first (tools/profile_round.sh -> tools/pmc_traffic.py)
LIVE_TRAFFIC = (None, "not attempted", 0.0)    # ({kernel: (read, write, launches)} | None, note, seconds): live_traffic_table
TRAFFIC_FILES = ("r06_pmc_traffic.json", "r05_pmc_traffic.json", "r04_pmc_traffic.json", "r03_pmc_traffic.json", "r02_pmc_traffic.json", "r01_pmc_traffic.json")
# algorithmic FLOPs of one 5-agent frame, points -> logits: encoder + decoder + heads, + one ConvGRU pass per GNN round
# (h0 = 0: W_hh is never multiplied and not counted)
GFLOP_PER_FRAME_BASE, GFLOP_PER_GNN_ROUND = 155.8, 36.2
# FLOPs the parity-class forms do NOT execute, per frame: (9 - 4) taps x upsampled channels x outputs x pixels x 2 x 5 agents -- conv8_1 (PARITY_CLASS >= 1),
# conv5_1 and conv6_1 (PARITY_CLASS >= 2), conv7_1 (PARITY_CLASS >= 3); each 6.71 GFLOP
GFLOP_PARITY_CLASS_SAVED = {0: 0.0, 1: 2 * AGENTS * 5 * 64 * 32 * 256 * 256 / 1e9,
                            2: 2 * AGENTS * 5 * (64 * 32 * 256 * 256 + 512 * 256 * 32 * 32 + 256 * 128 * 64 * 64) / 1e9,
                            3: 2 * AGENTS * 5 * (64 * 32 * 256 * 256 + 512 * 256 * 32 * 32 + 256 * 128 * 64 * 64 + 128 * 64 * 128 * 128) / 1e9}


def strip_kernel_args(name):
    """'void ns::k<a, b>(Args, (anonymous namespace)::T)' -> 'ns::k<a, b>': cut the ARGUMENT list = the parenthesis group that closes the string (matched
    from the right), not the first '(' (which may belong to '(anonymous namespace)::k')."""
    name = name.replace("void ", "", 1) if name.startswith("void ") else name
    name = name.rstrip()
    if not name.endswith(")"):
        return name
    depth = 0
    for i in range(len(name) - 1, -1, -1):
        if name[i] == ")":
            depth += 1
        elif name[i] == "(":
            depth -= 1
            if depth == 0:
                return name[:i].rstrip()
    return name


def live_traffic_wanted(args):
    """-> (True, "") or (False, why not).  The counter passes are children of a process that has NOT touched the GPU, never run under a profiler, never at
    N > 1, never from a rank child."""
    import shutil
    if args.no_live_traffic or args.no_roofline or os.environ.get("V2X_BENCH_LIVE_TRAFFIC", "1") == "0":
        return False, "switched off"
    if any(k.startswith(("ROCPROF", "ROCP_")) for k in os.environ) or "rocprofiler" in os.environ.get("LD_PRELOAD", ""):
        return False, "this run is itself under a profiler"
    if not os.path.exists(shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"):
        return False, "rocprofv3 not found"
    return True, ""


def live_traffic_table(args):
    """HBM bytes per launch of EVERY kernel of the step, MEASURED in this run: two child passes of this script under `rocprofv3 --pmc FETCH_SIZE` /
    `--pmc WRITE_SIZE` (separate passes, counters only -- no trace domain beside them; /opt/skills/guides/MI355X_MICROARCH.md, HBM section), 2 eager steps
    each, corrected as tools/pmc_traffic.py does (KiB -> bytes; FETCH_SIZE x 2 on gfx950).  Called from a process that has not touched the GPU (round 6:
    the N = 1 orchestrator, AFTER the timed run's child has exited -- the passes no longer pre-heat the chip before the timed region).
    Returns ({kernel: (read, write, launches)}, note, seconds) or (None, why not, seconds): any failure falls back to the committed profiles/ file."""
    import csv
    import glob
    import shutil
    import tempfile
    t_start = time.monotonic()
    ok, why = live_traffic_wanted(args)
    if not ok:
        return None, why, 0.0
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    table = {}
    timeout_s = float(os.environ.get("V2X_BENCH_PMC_TIMEOUT_S", "120"))
    for counter, factor in (("FETCH_SIZE", 1024.0), ("WRITE_SIZE", 1024.0)):       # KiB -> bytes; the FETCH_SIZE calibration factor is applied per kernel in apply_live_traffic
        out = tempfile.mkdtemp(prefix="v2x_pmc_", dir="/tmp")
        cmd = [rocprof, "--pmc", counter, "-d", out, "-o", "p", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
               "--steps", "2", "--warmup", "1", "--graph", "0", "--frames-per-gpu", str(args.frames_per_gpu), "--gnn-iters", str(args.gnn_iters)]
        env = dict(os.environ, TMPDIR="/tmp", V2X_BENCH_LIVE_TRAFFIC="0", V2X_BENCH_INNER="1")
        try:
            proc = subprocess.Popen(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, start_new_session=True)
            try:
                rc = proc.wait(timeout=timeout_s)
            except subprocess.TimeoutExpired:
                os.killpg(proc.pid, 9)
                proc.wait()
                return None, "the %s pass timed out (%.0f s)" % (counter, timeout_s), time.monotonic() - t_start
            # the bench child's file: the LARGEST counter_collection CSV under the output directory (a helper process of the child would leave a small one)
            files = sorted(glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True), key=os.path.getsize, reverse=True)
            if rc != 0 or not files:
                return None, "the %s pass failed (exit code %s)" % (counter, rc), time.monotonic() - t_start
            acc = {}
            with open(files[0]) as fh:
                for r in csv.DictReader(fh):
                    if r["Counter_Name"] != counter:
                        continue
                    e = acc.setdefault(strip_kernel_args(r["Kernel_Name"]), [0, 0.0])
                    e[0] += 1
                    e[1] += float(r["Counter_Value"])
            for name, (n, total) in acc.items():
                table.setdefault(name, {})[counter] = (factor * total / n, n)
        except Exception as e:      # noqa: BLE001 -- a measurement aid must never take the bench line down
            return None, "%s: %s" % (type(e).__name__, e), time.monotonic() - t_start
        finally:
            shutil.rmtree(out, ignore_errors=True)
    full = {k: (v["FETCH_SIZE"][0], v["WRITE_SIZE"][0], v["FETCH_SIZE"][1]) for k, v in table.items() if "FETCH_SIZE" in v and "WRITE_SIZE" in v}
    el = time.monotonic() - t_start
    return (full, "measured in this run", el) if full else (None, "no kernel in both passes", el)


def apply_live_traffic(roofline, live, when):
    """Put the in-run counter measurement of the dominant kernel into `roofline` (the committed value stays beside it as `traffic_committed`)."""
    table, note, seconds = live
    dom = roofline.get("kernel")
    if table is not None and dom in table:
        raw, wr, nl = table[dom]
        ff = FETCH_FACTOR.get(dom, FETCH_FACTOR_DEFAULT)
        rd = ff * raw
        roofline["traffic_committed"] = roofline.get("traffic")
        roofline["traffic"] = rd + wr
        roofline["traffic_uniform_x2"] = 2.0 * raw + wr           # rounds 2-5's convention (every kernel's FETCH_SIZE doubled), for continuity
        roofline["fetch_factor"] = ff
        roofline["fetch_factor_calibrated"] = dom in FETCH_FACTOR
        roofline["traffic_source"] = ("measured in this run: rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE child passes of this script %s "
                                      "(separate, counters only; 2 eager steps each, %d launches of the kernel averaged; KiB -> bytes; FETCH_SIZE x %.2f = this kernel's "
                                      "calibrated mix of wide reads (x 2, the guide's gfx950 correction) and 64-byte segment reads (x 1.1), profiles/r06_fetch_calibration.txt): "
                                      "read %.1f MB + write %.1f MB per launch" % (when, nl, ff, rd / 1e6, wr / 1e6))
        roofline.pop("traffic_live", None)
    else:
        roofline["traffic_live"] = "not re-measured: " + (note if table is None else "kernel not in the counter passes")
    roofline["pmc_passes_s"] = round(seconds, 1)
    return roofline


def orchestrate(args, argv):
    """N = 1 with the in-run traffic measurement on (the default): THIS process never touches the GPU.  It runs (1) the benchmark proper as a fresh child
    -- the timed region meets a chip nothing has warmed up, as the driver's clock expects -- then (2) the two rocprofv3 --pmc passes (fresh children
    again), and merges their result into the child's record.  Round 5 ran the passes BEFORE the timed run: ~40 s of work on a power / thermally limited
    chip right in front of a 0.4-s timed window (the paired runs are in profiles/r06_pmc_order_ab.txt)."""
    env = dict(os.environ, V2X_BENCH_INNER="1")
    proc = subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), stdout=subprocess.PIPE, text=True, env=env)
    record = None
    for line in proc.stdout:
        if line.startswith('{"metric"'):
            record = line.rstrip("\n")
        else:
            sys.stdout.write(line)
    rc = proc.wait()
    sys.stdout.flush()
    if record is None:
        if rc == 0:
            rc = 1
            print("bench.py: the benchmark child exited 0 without a JSON record", file=sys.stderr)
        return rc
    try:
        rec = json.loads(record)
        if isinstance(rec.get("roofline"), dict):
            apply_live_traffic(rec["roofline"], live_traffic_table(args), "AFTER the timed run (fresh child processes; the timed region met a cold chip)")
            rec["summary"] = rec.pop("summary", None)     # keep the compact summary the LAST key of the line
        record = json.dumps(rec)
    except Exception as e:      # noqa: BLE001 -- the child's record stands as it is
        print("bench.py: in-run traffic measurement skipped: %r" % (e,), file=sys.stderr)
    print(record, flush=True)
    return rc


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames-per-gpu", type=int, default=128,
                    help="frames per step and GPU (two half-batches of 64 = 320 maps: every conv layer then splits into a "
                         "whole number of rounds of 256 workgroups; 64 frames/GPU leaves the 32x32 layers at 2.5 rounds, -4 %%)")
    ap.add_argument("--gnn-iters", type=int, default=1)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run everything else the benchmark measures or checks (minutes): graph == eager and sharded == unsharded, "
                         "the instrumented roofline pass with its two counter passes, the calibration probes, latency / other configs / training / host streaming, "
                         "the stock PyTorch-ROCm and CPU baselines, the strong-scaling workload at N > 1.  Without it none of them runs and their keys in the "
                         "line are null; the --no-* options below drop single legs of a --full run")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-gpu-baseline", action="store_true", help="skip the same-node stock PyTorch-ROCm comparator (`gpu_stock_baseline`)")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-live-traffic", action="store_true",
                    help="do not re-measure the dominant kernel's HBM traffic with two rocprofv3 --pmc child passes (the committed profiles/ file is quoted instead)")
    ap.add_argument("--no-calibration", action="store_true", help="skip the streaming / MFMA calibration probes (the `calibration` sub-record)")
    ap.add_argument("--graph", type=int, default=1,
                    help="1: four hipGraph segments with the exchange between them, the two half-batches on two streams (every N); "
                         "4: the same on one stream; 0: eager launches; 2: the whole step as ONE hipGraph (N = 1 only, for comparison); "
                         "5 (experiment, round 6): as 1 but the two half-batch streams FREE-RUN over the timed steps (no join at the end of a step; "
                         "V2X_BENCH_STAGGER=1: half B starts one encoder behind half A) -- joined once, by the synchronize that ends the timed region")
    ap.add_argument("--transport", choices=("allgather", "needed"), default="allgather",
                    help="fusion-map exchange: RCCL all-gather (default) or grouped point-to-point of the needed rows only")
    ap.add_argument("--layout", choices=("spread", "agent-per-gpu"), default="spread",
                    help="spread (default): the agent-major (agent, frame) items in equal contiguous slices over ALL N ranks; "
                         "agent-per-gpu: the north_star's literal layout -- rank a < 5 owns agent a's frames, ranks >= 5 idle "
                         "(needs N >= 5; frames = frames_per_gpu * 5)")
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak",
                    help="weak (default, the headline): per-GPU work fixed, frames per step = frames_per_gpu * N; when N > 1 a --full run times the strong workload as "
                         "well and printed as the sub-record `strong`.  strong: total work fixed at frames_per_gpu frames per step whatever N")
    ap.add_argument("--no-shard-check", action="store_true", help="skip the sharded == unsharded recomputation after the timed region")
    ap.add_argument("--no-extras", action="store_true", help="skip the latency and other-config sub-records")
    ap.add_argument("--dry-run", action="store_true", help="no GPU: launcher, rendezvous (gloo), shard plan, collective, JSON relay")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the logits the last timed step computed (rank 0's items) to DIR/<name>.npy as float32: "
                         "item 0 of half-batch A whole and a fixed seeded sample of every half-batch's cls / loc (dump_outputs; under 64 MB in all)")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be >= 1 (the number of timed steps)")
    if not args.full:
        args.no_cpu_baseline = args.no_gpu_baseline = args.no_roofline = args.no_live_traffic = True
        args.no_calibration = args.no_shard_check = args.no_extras = True
    return args


def cpu_baseline(model_state, gnn_iters, budget_s=20.0):
    """Oracle V2VNet (PyTorch-CPU fp32 + numpy voxelizer) on whole 5-agent frames, same synthetic
    generator; at least 1 timed frame, stops after ~budget_s."""
    from oracle import coperception_ref as R
    from oracle import voxelize_ref as VR
    from v2x_sim_amd.utils.synthetic import synthetic_points, synthetic_poses
    # measured on the MI355X host (256 hardware threads): 8 thr 0.44, 16 thr 0.40, 32 thr 0.40,
    # 64 thr 0.79, 256 thr 45 s/frame -- oneDNN oversubscribes on this small batch, so cap at 32.
    cores = min(os.cpu_count() or 1, 32)
    torch.set_num_threads(cores)
    om = R.V2VNet(gnn_iter_times=gnn_iters).eval()
    om.load_state_dict(model_state)
    pts = synthetic_points(AGENTS, POINTS_PER_SWEEP, seed=1234)
    T = torch.from_numpy(synthetic_poses(1, AGENTS, seed=99))
    nat = torch.full((1, AGENTS), AGENTS)

    def frame():
        bev = np.stack([VR.voxelize_occupy(p) for p in pts])[:, None]
        with torch.no_grad():
            om(torch.from_numpy(bev), T, nat, batch_size=1)

    frame()  # warm-up (oneDNN primitive setup)
    n, t0 = 0, time.perf_counter()
    while True:
        frame()
        n += 1
        el = time.perf_counter() - t0
        if el > budget_s or n >= 40:
            break
    rec = {"value": n / el, "unit": "frames/s", "cores": cores, "kind": "port",
           "sample": "%d whole 5-agent V2VNet frames (65536 pts/agent, 256x256x13 BEV), oracle fp32 PyTorch-CPU, "
                     "%d threads, after 1 warm-up frame" % (n, torch.get_num_threads())}
    # BASELINE.json config 0 AS WRITTEN -- "lowerbound (no-fusion) single-agent BEV detection on PyTorch CPU" -- is a CPU run of the reference; the product has no CPU
    # path, so that config exists here only as the ORACLE's lowerbound network on these host cores (VERDICT r5 missing #5): the same five sweeps, no fusion stage
    try:
        lo = R.FaFNet().eval()
        ren = lambda k: "stpn.encoder." + k[len("u_encoder."):] if k.startswith("u_encoder.") else ("stpn.decoder." + k[len("decoder."):] if k.startswith("decoder.") else k)   # noqa: E731
        lo.load_state_dict({ren(k): v for k, v in model_state.items() if not k.startswith("convgru")})     # the V2VNet's own backbone and heads, minus its fusion stage

        def lo_frame():
            bev = np.stack([VR.voxelize_occupy(p) for p in pts])[:, None]
            with torch.no_grad():
                lo(torch.from_numpy(bev))
        lo_frame()
        m, t1 = 0, time.perf_counter()
        while True:
            lo_frame()
            m += 1
            el2 = time.perf_counter() - t1
            if el2 > budget_s / 3.0 or m >= 20:
                break
        rec["config0_lowerbound_on_cpu"] = {"frames_per_s": m / el2, "frames": m, "what": "oracle FaFNet (lowerbound: no fusion), 5 agents per frame, fp32 PyTorch-CPU, %d threads" % torch.get_num_threads()}
    except Exception as e:      # noqa: BLE001
        rec["config0_lowerbound_on_cpu"] = {"error": repr(e)[:200]}
    return rec


def gpu_stock_baseline(model_state, gnn_iters, dev, frames=64, reps=10, warm=3):
    """The SAME-NODE comparator: the reference's execution model is stock PyTorch on the GPU (/root/reference/README.md:88-95:
    PyTorch 1.8 + CUDA 11.2) -- on this node PyTorch-ROCm with MIOpen convolutions.  The oracle V2VNet (oracle/coperception_ref.py, the restated
    upstream graph incl. its per-pair warp loop and batch-1 ConvGRU calls) is moved to cuda:0 and timed on one 64-frame half-batch of dense BEV
    voxels under torch.no_grad(): (i) fp32, (ii) bf16 autocast + channels_last.  Median of `reps` after `warm` warm-ups.  Bench-side only: never in
    the product, never in the timed region; voxelisation excluded (the reference does it on the CPU in its DataLoader).  The pose matrices stay on
    the host, so the warp loop's scalar reads do not synchronise the device (kinder to the stock path than upstream's device-resident matrices)."""
    from oracle import coperception_ref as R
    from v2x_sim_amd.utils.synthetic import synthetic_poses
    out = {"frames": frames, "maps": frames * AGENTS, "unit": "frames/s", "reps": reps, "warmups": warm,
           "what": "stock PyTorch-ROCm (MIOpen convolutions, aten grid_sample), the reference's execution model per /root/reference/README.md:88-95: "
                   "the oracle V2VNet graph on cuda:0, dense BEV voxels -> logits, torch.no_grad(), median of %d after %d warm-ups" % (reps, warm)}
    om = R.V2VNet(gnn_iter_times=gnn_iters).eval()
    om.load_state_dict(model_state)
    om = om.to(dev)
    g = torch.Generator(device="cpu").manual_seed(4321)
    bev = (torch.rand((AGENTS * frames, 1, 256, 256, 13), generator=g) < 0.03).to(torch.float32).to(dev)     # ~3 % occupancy, as a sweep leaves
    T = torch.from_numpy(synthetic_poses(frames, AGENTS, seed=99))         # host-resident on purpose (see above)
    nat = torch.full((frames, AGENTS), AGENTS)

    def timed(fn):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        ts.sort()
        return ts[len(ts) // 2]

    def fp32():
        with torch.no_grad():
            om(bev, T, nat, batch_size=frames)

    def bf16():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            om(bev, T, nat, batch_size=frames)
    def to_channels_last():         # the 2-D convolutions' weights only (nn.Module.to(memory_format=) refuses the model's 5-D Conv3d weights)
        for m in om.modules():
            if isinstance(m, torch.nn.Conv2d):
                m.weight.data = m.weight.data.contiguous(memory_format=torch.channels_last)
    for key, fn, prep in (("fp32", fp32, None), ("bf16_autocast_channels_last", bf16, to_channels_last)):
        try:
            if prep is not None:
                prep()
            t = timed(fn)
            out[key + "_ms"] = t * 1e3
            out[key + "_frames_per_s"] = frames / t
        except Exception as e:      # noqa: BLE001 -- a side baseline must not take the record down
            out[key + "_error"] = repr(e)[:300]
    best = max([out.get("fp32_frames_per_s") or 0.0, out.get("bf16_autocast_channels_last_frames_per_s") or 0.0])
    out["value"] = best or None
    del om, bev
    torch.cuda.empty_cache()
    return out


# forward FLOPs of one (agent, frame) map in the reference's arithmetic: encoder + decoder + heads = 31.16 GFLOP; V2VNet adds one ConvGRU pass
TRAIN_FWD_GFLOP_PER_MAP = {"FaFNet": GFLOP_PER_FRAME_BASE / AGENTS, "V2VNet": (GFLOP_PER_FRAME_BASE + GFLOP_PER_GNN_ROUND) / AGENTS}


def training_fractions(training):
    """Row f-3's roofline: a training step = forward + data gradient + weight gradient ~ 3 x the forward FLOPs (the convolutions are
    >99 % of them) -> 3 x GFLOP per map x maps / step time in ms (= TFLOP/s) / 2 500 TFLOP/s, for the HIP engine's fastest form at 10, 20 and 40 maps."""
    out = {}
    try:
        m10 = training.get("maps_per_step", 10)
        for name in ("FaFNet", "V2VNet"):
            rec = training.get(name) or {}
            ms = [v for k, v in rec.items() if ("hipGraph" in k or "HIP kernels" in k) and isinstance(v, (int, float))]
            if ms:
                out["%s_%d_maps" % (name, m10)] = 3.0 * TRAIN_FWD_GFLOP_PER_MAP[name] * m10 / min(ms) / PEAK_MFMA_TFLOPS
        for key, rec in training.items():
            if key.startswith("maps_") and isinstance(rec, dict):
                maps = int(key.split("_")[1])
                for k, v in rec.items():
                    name = k.split(" ")[0]
                    if name in TRAIN_FWD_GFLOP_PER_MAP and isinstance(v, (int, float)):
                        out["%s_%d_maps" % (name, maps)] = 3.0 * TRAIN_FWD_GFLOP_PER_MAP[name] * maps / v / PEAK_MFMA_TFLOPS
    except Exception as e:      # noqa: BLE001
        out["error"] = repr(e)
    return out


def build_summary(fps, ms_per_step, latency, configs, training, gpu_stock, cpu, roofline, executed_gflop, world):
    """The numbers BASELINE.md section 3 asks for, flat and short (scalars only, so that a parser that drops nested records keeps them)."""
    sm = {"headline_frames_per_s": fps, "headline_ms_per_step": ms_per_step}
    if isinstance(latency, dict):
        for b in (1, 8, 32):
            if "b%d_ms" % b in latency:
                sm["latency_b%d_ms" % b] = latency["b%d_ms" % b]
                sm["latency_b%d_frames_per_s" % b] = latency["b%d_frames_per_s" % b]
    if isinstance(configs, dict) and isinstance(configs.get("configs"), dict):
        short = {"0n": "config0_lowerbound_net", "1": "config1_upperbound", "2": "config2_v2vnet", "2d": "config2_points_to_detections", "3": "config3_when2com",
                 "3b": "config3b_who2com", "4": "config4_v2vnet_seg"}
        for k, v in configs["configs"].items():
            tag = short.get(k.split(" ")[0])
            if tag and isinstance(v, dict):
                sm[tag + "_frames_per_s"] = v.get("frames_per_s")
    if isinstance(gpu_stock, dict):
        sm["gpu_stock_fp32_frames_per_s"] = gpu_stock.get("fp32_frames_per_s")
        sm["gpu_stock_bf16_frames_per_s"] = gpu_stock.get("bf16_autocast_channels_last_frames_per_s")
        if gpu_stock.get("value"):
            sm["speedup_vs_gpu_stock"] = fps / world / gpu_stock["value"]
    if isinstance(cpu, dict) and cpu.get("value"):
        sm["speedup_vs_cpu_baseline"] = fps / world / cpu["value"]
    if isinstance(training, dict) and isinstance(training.get("frac_of_mfma_peak"), dict):
        for k, v in training["frac_of_mfma_peak"].items():
            if isinstance(v, float):
                sm["train_frac_" + k] = round(v, 4)
    if isinstance(roofline, dict):
        sm["roofline_frac"] = roofline.get("frac")
    sm["whole_step_frac"] = executed_gflop * 1e9 * fps / world / (PEAK_MFMA_TFLOPS * 1e12)
    return sm


def stream_ceiling_fractions(kernels, calibration):
    """The HBM-side kernels against what a pure streaming kernel sustains ON THIS BOX at their read : write mix (calibration: v2x_calib_stream): the fused tail writes
    3 bytes per byte it reads (fp32 logits), conv8_1 (parity-class) reads 2 : writes 1, conv1_1 reads 4 : writes 1 ... -> {kernel: algorithmic GB/s / ceiling}.  A value
    near 1 means the kernel already moves its algorithmic bytes as fast as memory takes that mix -- VERDICT r5's "tail <= 1 100 us" asks for 4.9 TB/s at 1 : 3, above it."""
    mixes = {"conv3x3_tail_kernel": "copy_1_3_tbs", "conv3x3_halo_ppc_kernel<64, 32, 32>": "copy_2_1_tbs", "conv3x3_s2_resident_kernel<64>": "copy_4_1_tbs",
             "conv3x3_halo_sb_kernel<0, 32, 32, 0, 0, false>": "copy_1_1_tbs", "conv3x3_halo_pp_kernel<0, 64, 64, 0>": "copy_1_1_tbs"}
    out = {}
    if isinstance(kernels, dict) and isinstance(calibration, dict):
        for k, key in mixes.items():
            if k in kernels and calibration.get(key):
                out[k] = {"mix": key[5:-4].replace("_", ":"), "algorithmic_tb_s": kernels[k]["gbs"] / 1e3, "stream_ceiling_tb_s": calibration[key],
                          "frac": kernels[k]["gbs"] / 1e3 / calibration[key]}
    return out


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(args, argv):
    """Parent of an N > 1 run started as plain `python bench.py --gpus N`: starts the ranks as CHILD processes through
    torch.distributed.run (one per GPU, RCCL over xGMI; 127.0.0.1 rendezvous) and relays their output.  Nothing here
    touches the GPU -- a process that has initialised HIP must never be re-exec'd or forked into ranks."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % args.gpus,
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "4")
    env.setdefault("V2X_BENCH_PORT2", str(_free_port()))     # the rendezvous port of a relaunch (supervise), chosen HERE while it is known to be free
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, env=env)
    record = None
    for line in proc.stdout:
        if line.startswith('{"metric"'):
            record = line.rstrip("\n")          # printed last, after everything else the ranks wrote
        else:
            sys.stdout.write(line)
    rc = proc.wait()
    sys.stdout.flush()
    if record is not None:
        print(record, flush=True)
    elif rc == 0:
        rc = 1
        print("bench.py: the ranks exited 0 without a JSON record", file=sys.stderr)
    return rc


# ---- watchdog around a rank (N > 1 only) -----------------------------------------------------------------------------------------------
# The first N > 1 run on hardware is the driver's, not ours (no multi-GPU node was ever available to this build): the default execution -- two
# half-batch streams, each issuing asynchronous RCCL collectives in host order -- has only ever met a 1-rank group.  So every rank process the
# launcher starts is a SUPERVISOR that has not touched the GPU: it runs the actual rank as a CHILD process (never a re-exec of a process that
# initialised HIP) and watches two markers on the child's stdout -- "ranks-ready" (model, data and process group built: the next thing is the
# first step with collectives) and "first-step-done" (warm-up, capture and the first replayed step are behind every rank: printed after a
# job-wide barrier).  If rank 0's child does not get from the
# first marker to the second within V2X_BENCH_WATCHDOG_S (default 240 s), rank 0's supervisor raises a node-local flag file; every supervisor polls
# it, kills its child (its whole process group) and starts a FRESH child in the conservative order `--graph 4` (one stream: strictly sequential
# collectives) on another rendezvous port (chosen free by launch_ranks: V2X_BENCH_PORT2).  The record says which attempt produced it (`launch`).
# One relaunch only: a second stall -- seen by EVERY rank through a second flag -- exits 124, and so does a run that exceeds V2X_BENCH_TOTAL_S
# (default 1500 s) after its first step: slow is not stalled, that run is not started again (round 6).
MARK_READY, MARK_FIRST = "#v2x-bench ranks-ready", "#v2x-bench first-step-done"


def _mark(text, use_dist=False):
    """Child side: a progress marker for the supervisor (a plain stdout line; the supervisor filters it out)."""
    if os.environ.get("V2X_BENCH_CHILD") == "1":
        if use_dist and dist.is_initialized():
            dist.barrier()
        print(text, flush=True)


def supervise(args, argv, rank, world):
    import signal
    import threading
    watchdog_s = float(os.environ.get("V2X_BENCH_WATCHDOG_S", "240"))
    total_s = float(os.environ.get("V2X_BENCH_TOTAL_S", "1500"))
    base_port = int(os.environ.get("MASTER_PORT", "29531"))
    port2 = int(os.environ.get("V2X_BENCH_PORT2", str(base_port + 17)))     # launch_ranks picks a free one; under a foreign launcher: a fixed offset
    # node-local flag files, named by a per-LAUNCH nonce every supervisor of this launch derives alike: the launcher's pid AND its start time (a stale
    # file of an earlier launch that re-used pid and port cannot be mistaken for this launch's)
    ppid = os.getppid()
    try:
        with open("/proc/%d/stat" % ppid) as fh:
            born = fh.read().rsplit(")", 1)[1].split()[19]
    except Exception:       # noqa: BLE001
        born = "0"
    stem = os.path.join(os.environ.get("TMPDIR", "/tmp"), "v2x_bench_%d_%d_%s" % (base_port, ppid if "TORCHELASTIC_RUN_ID" in os.environ else 0, born))
    flag, flag2 = stem + "_relaunch", stem + "_abort"
    if rank == 0:
        for f in (flag, flag2):
            if os.path.exists(f):
                os.unlink(f)
    rc = 1
    for attempt in (1, 2):
        env = dict(os.environ)
        env["V2X_BENCH_CHILD"] = "1"
        env["V2X_BENCH_ATTEMPT"] = str(attempt)
        if attempt == 2:
            # a fresh rendezvous: another port, and rank 0's child hosts the store itself (under torchrun the agent hosts the store of the FIRST
            # rendezvous on MASTER_PORT -- TORCHELASTIC_USE_AGENT_STORE -- and its keys belong to the killed attempt)
            env["MASTER_PORT"] = str(port2)
            env["TORCHELASTIC_USE_AGENT_STORE"] = "False"
        extra = [] if attempt == 1 else ["--graph", "4"]
        proc = subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv) + extra, stdout=subprocess.PIPE, text=True, env=env,
                                start_new_session=True)
        state = {"ready": None, "first": None, "record": None}

        def reap(signum, _frame, p=proc):     # the launcher (or a timeout) is taking this supervisor down: the child (own session) goes with it
            try:
                os.killpg(p.pid, signal.SIGKILL)
            except ProcessLookupError:
                pass
            sys.exit(128 + signum)
        for sg in (signal.SIGTERM, signal.SIGINT, signal.SIGHUP):
            signal.signal(sg, reap)

        def pump(p=proc, st=state):
            for line in p.stdout:
                if line.startswith(MARK_READY):
                    st["ready"] = time.monotonic()
                elif line.startswith(MARK_FIRST):
                    st["first"] = time.monotonic()
                else:
                    sys.stdout.write(line)
                    sys.stdout.flush()
        th = threading.Thread(target=pump, daemon=True)
        th.start()
        t0 = time.monotonic()
        stalled = over_budget = False
        while proc.poll() is None:
            time.sleep(0.25)
            now = time.monotonic()
            if os.path.exists(flag2):                   # rank 0 gave the whole job up (total budget, or a second stall): no relaunch
                stalled = over_budget = True
            elif attempt == 1 and os.path.exists(flag):
                stalled = True
            elif rank == 0 and state["ready"] is not None and state["first"] is None and now - state["ready"] > watchdog_s:
                stalled = True                          # the first step with collectives did not complete: the ONLY condition that relaunches
                open(flag if attempt == 1 else flag2, "w").write("stalled after %.0f s\n" % (now - t0))
            elif rank == 0 and now - t0 > total_s:
                # a healthy but slow run is not a stall: give up with 124, do not start the whole bench again in another order
                stalled = over_budget = True
                open(flag2, "w").write("total budget of %.0f s spent\n" % total_s)
            if stalled:
                print("bench.py: rank %d: attempt %d %s -> killing the rank process%s" % (
                    rank, attempt, "over the total budget of %.0f s" % total_s if over_budget and state["first"] is not None else
                    "stalled (no first step within %.0f s of ranks-ready)" % watchdog_s,
                    " and relaunching with --graph 4" if attempt == 1 and not over_budget else ""), file=sys.stderr, flush=True)
                try:
                    os.killpg(proc.pid, signal.SIGKILL)
                except ProcessLookupError:
                    pass
                proc.wait()
                break
        th.join(timeout=5)
        rc = proc.returncode if not stalled else 124
        if not stalled or attempt == 2 or over_budget:
            break
        time.sleep(1.0)     # every supervisor has seen the flag and killed its child before the new rendezvous starts
    if rank == 0:
        time.sleep(1.0)
        for f in (flag, flag2):
            if os.path.exists(f):
                os.unlink(f)
    return rc


def shard_layout(args, world, rank):
    """-> (shard_world, shard_rank or None for an idle rank, process group of the shard or None = the default group).
    `agent-per-gpu` runs the 5 agents on ranks 0..4 of the job (their own sub-group, created collectively by ALL ranks); the other
    ranks only take part in the job-wide barriers and the max-over-ranks timing."""
    if args.layout == "spread":
        return world, rank, None
    if world < AGENTS:
        raise SystemExit("--layout agent-per-gpu needs --gpus >= %d (one GPU per agent)" % AGENTS)
    group = dist.new_group(ranks=list(range(AGENTS))) if world > AGENTS else None
    return AGENTS, (rank if rank < AGENTS else None), group


def launch_record(args):
    """How this rank process was started: directly, or as the child of a supervisor (attempt 2 = after a stalled first attempt, --graph 4)."""
    return {"supervised": os.environ.get("V2X_BENCH_CHILD") == "1", "attempt": int(os.environ.get("V2X_BENCH_ATTEMPT", "1")),
            "graph_mode": args.graph, "watchdog_s": float(os.environ.get("V2X_BENCH_WATCHDOG_S", "240"))}


def dry_run(args, world, rank):
    """CPU walk through everything around the kernels: rendezvous, agent-major partition, fusion plan, the exchange
    calls (gloo instead of RCCL), barrier + max-over-ranks timing, one JSON line from rank 0."""
    from v2x_sim_amd.parallel import AgentShard, ShardedV2VNet
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29531")
        dist.init_process_group("gloo", rank=rank, world_size=world)
    sworld, srank, group = shard_layout(args, world, rank)
    Bh = args.frames_per_gpu * sworld // 2
    ok = torch.tensor([1])
    t0 = time.perf_counter()
    per_rank = AGENTS * Bh // sworld
    if srank is not None:
        shard = AgentShard(AGENTS, Bh, srank, sworld)

        class _NoModel:
            gnn_iter_num, neighbor_source, layer = 1, "initial", 3
        runner = ShardedV2VNet(_NoModel(), shard, group=group, transport=args.transport)
        plan = shard.fusion_plan(torch.full((Bh, AGENTS), AGENTS), "cpu")
        local = torch.stack([torch.full((2, 2, 8), float(r)) for r in shard.rows])  # fp32: row ids beyond 256 stay exact
    _mark(MARK_READY)
    # test hooks: V2X_BENCH_DELAY_RANK / _S = that rank sleeps before its FIRST exchange (a late rank must only delay, never deadlock, the
    # two-stream host order below); V2X_BENCH_SIMULATE_HANG = that rank never issues its first exchange in attempt 1 (a stuck collective)
    delay_rank = int(os.environ.get("V2X_BENCH_DELAY_RANK", "-1"))
    hang_rank = int(os.environ.get("V2X_BENCH_SIMULATE_HANG", "-1")) if os.environ.get("V2X_BENCH_ATTEMPT", "1") == "1" else -1
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    if srank is not None:
        for it in range(args.steps):
            if it == 0 and rank == hang_rank:
                time.sleep(3600)
            if it == 0 and rank == delay_rank:
                time.sleep(float(os.environ.get("V2X_BENCH_DELAY_S", "2")))
            # the host order of bench.py's default step (Workload.build, mode 1): encoder A, exchange A (async), encoder B, exchange B (async),
            # then wait A + decode A, wait B + decode B -- both exchanges are in flight before either is waited for, in the same order on every rank
            ga, wa = runner.start_exchange(local)
            gb, wb = runner.start_exchange(local + 0.5)
            runner.wait(wa)
            runner.wait(wb)
            gathered = ga
            ok = torch.minimum(ok, torch.tensor([int(bool(torch.equal(gb, ga + 0.5)))]))
    if world > 1:
        dist.barrier()
    _mark(MARK_FIRST)       # (after the job-wide barrier: idle ranks of the agent-per-gpu layout take part in it, not in the exchanges)
    t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    if srank is not None:
        # every map an owned ego reads (all agents of its frame) must sit at its agent-major row
        ok = torch.tensor([int(all(float(gathered[j * Bh + f, 0, 0, 0]) == j * Bh + f
                                   for _, f in plan["items"].tolist() for j in range(AGENTS)))])
    # the rows bench.py's sharded == unsharded self-check would compare on this rank, at the weak and the strong geometry
    n_pairs = None
    if srank is not None:
        n_pairs = []
        for bh in (Bh, args.frames_per_gpu // 2):
            if (AGENTS * bh) % sworld == 0:
                rows = AgentShard(AGENTS, bh, srank, sworld).rows
                frames, pairs = shard_check_plan(rows, bh)
                good = bool(pairs) and all(rows[gi] == (ri // len(frames)) * bh + frames[ri % len(frames)] for ri, gi in pairs)
                ok = torch.minimum(ok, torch.tensor([int(good)]))
                n_pairs.append(len(pairs))
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps({"metric": "BEV frames/sec, V2VNet 5-agent detection (256x256 BEV)", "value": None, "unit": "frames/s",
                          "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "dry_run": True, "ranks_seen": world,
                          "exchange_ok": bool(int(ok)), "transport": args.transport, "layout": args.layout, "active_ranks": sworld,
                          "frames_per_step": 2 * Bh, "items_per_rank": per_rank, "elapsed_s": float(t),
                          "strong_items_per_rank": (AGENTS * (args.frames_per_gpu // 2)) // sworld if (AGENTS * (args.frames_per_gpu // 2)) % sworld == 0 else None,
                          "shard_check_pairs": n_pairs, "launch": launch_record(args)}), flush=True)
    return 0 if int(ok) else 1


def measure_latency(model, dev, frames_list=(1, 8, 32), reps=30, small_batch=True):
    """Latency mode (SURVEY.md 8d batch sizes): ONE hipGraph replay of points -> logits for `frames` collaborative frames, host-synchronised per
    replay, median over `reps`.  small_batch=True: the sharded runner with the tuning switch SMALL_BATCH pinned to 1 (split-K for the streamed
    layers whose launch has fewer tiles than CUs, v2x_sim_amd/ops.py::small_batch_splitk) -- what a sharded server turns on.  small_batch=False
    ("default_dispatch"): the PLAIN model class out of the box -- model.forward_points(...) under the default tuning, which declares latency
    launches by itself (SMALL_BATCH = 2)."""
    from v2x_sim_amd import tuning
    prev = tuning.get("SMALL_BATCH")
    if small_batch:
        tuning.set("SMALL_BATCH", 1)
    try:
        return _measure_latency(model, dev, frames_list, reps, small_batch)
    finally:
        tuning.set("SMALL_BATCH", prev)


def _measure_latency(model, dev, frames_list, reps, small_batch):
    from v2x_sim_amd.parallel import AgentShard, ShardedV2VNet
    from v2x_sim_amd.utils.synthetic import synthetic_points, synthetic_poses
    out = {}
    for frames in frames_list:
        sh = AgentShard(AGENTS, frames, 0, 1)
        rn = ShardedV2VNet(model, sh)
        pts = torch.from_numpy(np.concatenate([synthetic_points(1, POINTS_PER_SWEEP, seed=5000 + r) for r in sh.rows])).to(dev)
        n_pts = torch.full((sh.per_rank,), POINTS_PER_SWEEP, dtype=torch.int32, device=dev)
        trans = torch.from_numpy(synthetic_poses(frames, AGENTS, seed=7)).to(dev)
        nat = torch.full((frames, AGENTS), AGENTS)
        if small_batch:
            plan = sh.fusion_plan(nat, dev)
            fwd = lambda: rn.forward_points(pts, n_pts, trans, plan)     # noqa: E731
        else:
            plan = model.make_plan(nat, frames, dev)
            fwd = lambda: model.forward_points(pts, n_pts, trans, nat, batch_size=frames, plan=plan)     # noqa: E731
        with torch.no_grad():
            for _ in range(2):
                fwd()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                res = fwd()
        for _ in range(3):
            g.replay()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            g.replay()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        out["b%d_ms" % frames] = ts[len(ts) // 2]
        out["b%d_frames_per_s" % frames] = frames / ts[len(ts) // 2] * 1e3
        del g, res
    out["mode"] = "one hipGraph replay of points->logits per batch, host-synchronised, median of %d; %s" % (
        reps, "sharded runner, SMALL_BATCH = 1 (split-K for launches with fewer tiles than CUs)" if small_batch else
        "the plain model class out of the box: V2VNet.forward_points under the default tuning (SMALL_BATCH = 2: it declares latency launches itself)")
    return out


def shard_check_plan(rows, Bh, n_frames=8):
    """Which frames a rank recomputes unsharded, and which of its items they cover.  rows: the GLOBAL agent-major rows (agent * Bh + frame) the
    rank owns in a half-batch of Bh frames.  -> (frames, pairs): `frames` = n_frames consecutive frames starting at the frame of the rank's first
    item (wrapping); pairs = [(row in the unsharded n_frames-batch = agent * n_frames + k, index into the rank's own output rows)] for every
    (agent, frames[k]) the rank owns -- never empty (the first item is always covered).  Pure host logic (tests/test_bench_launcher_cpu.py)."""
    n_frames = min(n_frames, Bh)
    f0 = rows[0] % Bh
    frames = [(f0 + k) % Bh for k in range(n_frames)]
    own = {r: i for i, r in enumerate(rows)}
    pairs = [(a * n_frames + k, own[a * Bh + frames[k]]) for a in range(AGENTS) for k in range(n_frames) if a * Bh + frames[k] in own]
    return frames, pairs


DUMP_SAMPLE = 1 << 21          # elements per sampled array (8 MB as float32)
DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(outs, out_dir):
    """--dump-outputs: what the timed path returned in its last step, for comparing two builds output for output.  `outs` = the per-half-batch
    {'cls', 'loc'} of this rank's items (Workload.outputs).  Written as float32 .npy: `<key>_item0` = item 0 of half-batch A whole, and
    `<key>_<half>_sample` = the elements at DUMP_SAMPLE sorted flat indices drawn from a generator seeded by (half, key) -- the same
    indices in every run with the same arguments (the whole output is ~8 GB at the default workload).  -> {name: shape}"""
    arrays = {}
    for hi, (half, out) in enumerate(zip("ab", outs)):
        for ki, key in enumerate(("cls", "loc")):
            x = out[key]
            if hi == 0:
                arrays["%s_item0" % key] = x[0]
            flat = x.reshape(-1)
            idx = np.sort(np.random.default_rng([hi, ki]).integers(0, flat.numel(), DUMP_SAMPLE))
            arrays["%s_%s_sample" % (key, half)] = flat[torch.from_numpy(idx).to(flat.device)]
    total = sum(4 * v.numel() for v in arrays.values())
    assert total <= DUMP_LIMIT_BYTES, total
    os.makedirs(out_dir, exist_ok=True)
    for name, v in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), v.detach().float().cpu().numpy())
    print("bench.py: %d output arrays (%.1f MB) written to %s" % (len(arrays), total / 2**20, out_dir), file=sys.stderr, flush=True)
    return {name: tuple(v.shape) for name, v in arrays.items()}


class Workload:
    """One benchmark workload: `frames_total` synthetic 5-agent frames per step over the whole job, run as two half-batches, agent-sharded over the
    active ranks (v2x_sim_amd/parallel.py).  measure() = warm-up, hipGraph capture, the timed K steps between barriers, then (--full) the correctness
    checks of what was timed: graph == eager (N = 1) and sharded == unsharded (every N; below)."""

    def __init__(self, ctx, frames_total, capture=True):
        from v2x_sim_amd.parallel import AgentShard, ShardedV2VNet
        from v2x_sim_amd.utils.synthetic import synthetic_points, synthetic_poses
        self.__dict__.update(ctx)
        args, dev, model = self.args, self.dev, self.model
        self.capture = capture
        self.Bt = frames_total                      # frames per step, whole job
        self.Bh = Bh = frames_total // 2            # frames per half-batch
        self.L = model.layer
        # The step is two independent half-batches of Bh frames, each agent-sharded over all ranks.  Half A's exchange
        # is started asynchronously and flies under half B's encoder; half B's flies under half A's fusion/decoder/heads.
        # The decomposition is the same for every N (at N = 1 there is simply nothing to gather).
        self.shard = shard = AgentShard(AGENTS, Bh, self.srank if self.active else 0, self.sworld)   # (an idle rank builds rank 0's tables and never launches)
        self.runner = ShardedV2VNet(model, shard, group=self.sgroup, transport=args.transport)
        if self.force_dist and self.world == 1:
            class _ForcedWorld1(ShardedV2VNet):     # take the world > 1 code path (async RCCL all-gather) on one rank
                def start_exchange(self, local, out=None, counts=None):
                    local = local.contiguous()
                    out = torch.empty_like(local) if out is None else out
                    return out, dist.all_gather_into_tensor(out, local, async_op=True)
            self.runner = _ForcedWorld1(model, shard)
        self.halves = []
        for h in range(2 if self.active else 0):
            # synthetic sweeps of this rank's (agent, frame) items of half h, resident in HBM; the seed of an item is a function of its GLOBAL row,
            # so that any rank can regenerate any item (check_sharding below)
            pts = np.concatenate([synthetic_points(1, POINTS_PER_SWEEP, seed=self.point_seed(h, r)) for r in shard.rows])
            self.halves.append({"points": torch.from_numpy(pts).to(dev),
                                "n_pts": torch.full((shard.per_rank,), POINTS_PER_SWEEP, dtype=torch.int32, device=dev),
                                "trans": torch.from_numpy(synthetic_poses(Bh, AGENTS, seed=99 + h)).to(dev),
                                "plan": shard.fusion_plan(torch.full((Bh, AGENTS), AGENTS), dev)})
        self.wait_events = []    # (start, end) HIP events around the stream-level wait for an exchange: the EXPOSED part of it
        self.mode = args.graph if self.active else -1
        self.exec_mode = None
        self.run = None

    @staticmethod
    def point_seed(h, row):
        return 1000 + 100000 * h + row

    def timed_wait(self, work):
        if work is None:
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.runner.wait(work)
        e1.record()
        self.wait_events.append((e0, e1))

    def step(self):
        runner = self.runner
        with torch.no_grad():
            a, b = self.halves
            fa, ga, wa = runner.begin(a["points"], a["n_pts"])
            fb, gb, wb = runner.begin(b["points"], b["n_pts"])
            self.timed_wait(wa)
            out_a = runner.decode(fa, ga, a["trans"], a["plan"])
            self.timed_wait(wb)
            out_b = runner.decode(fb, gb, b["trans"], b["plan"])
            return out_a, out_b

    def barrier(self):
        if self.use_dist:
            dist.barrier()

    def release(self):
        """Drop the graphs and buffers (the next workload / the extras build their own)."""
        for h in self.halves:
            for k in ("g_enc", "g_dec", "feats", "out", "xbuf", "points"):
                h.pop(k, None)
        self.run = self.last_out = None
        torch.cuda.empty_cache()

    def build(self):
        args, dev, runner, halves, shard, L = self.args, self.dev, self.runner, self.halves, self.shard, self.L
        use_dist, mode = self.use_dist, self.mode
        for _ in range((max(args.warmup, 1) if args.graph else args.warmup) if self.active else 0):
            self.last_out = self.step()
        torch.cuda.synchronize()
        self.barrier()          # every rank's warm-up collectives are finished before anybody starts capturing
        self.wait_events.clear()
        if mode == 2 and use_dist:
            raise SystemExit("--graph 2 (whole step in one hipGraph) is for N = 1 without V2X_FORCE_DIST")
        if mode == 2:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self.last_out = self.step()
            self.run = g.replay
            self._g = g
            self.exec_mode = "one hipGraph per step"
        elif mode in (1, 4, 5):
            # four collective-free segments (encoder A, encoder B, fusion + decoder + heads A, B), each a hipGraph; the exchange (RCCL, eager) runs
            # between them on static buffers.  mode 1 (default): the two half-batches on TWO STREAMS -- kernels of one half fill the tails and the
            # HBM-bound phases (heads, conv8_2, conv1_1) of the other: +2.3...3.0 % at N = 1 against the one-stream order (mode 4), same box;
            # four quarter-batches on four streams: -1.4 %.  The halves of a step are joined before the next step starts.
            # capture_error_mode="thread_local": RCCL's watchdog thread polls the events of earlier collectives while this
            # thread captures -- under the default global mode that query is "operation not permitted when stream is
            # capturing" and takes the process down (seen with V2X_FORCE_DIST=1 on one GPU)
            two = mode in (1, 5)
            free_run = mode == 5                       # no join at the end of a step: the streams drift / stay staggered; the device synchronize after the K steps joins them
            stagger = free_run and os.environ.get("V2X_BENCH_STAGGER", "0") == "1"
            self._stagger_armed = stagger
            shared_pool = torch.cuda.graph_pool_handle()
            streams = [torch.cuda.Stream(), torch.cuda.Stream()] if two else [torch.cuda.current_stream()] * 2
            with torch.no_grad():
                for h, st in zip(halves, streams):
                    h["xbuf"] = None
                    h["stream"] = st
                    # concurrent halves must not share intermediate buffers: one memory pool per half (one-stream order: one pool, replayed in capture order)
                    h["cap"] = dict(pool=torch.cuda.graph_pool_handle() if two else shared_pool, capture_error_mode="thread_local")
                    if use_dist:
                        h["xbuf"] = torch.empty((self.sworld * shard.per_rank, 32, 32, 256), dtype=torch.bfloat16, device=dev)
                for h in halves:
                    h["g_enc"] = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(h["g_enc"], **h["cap"]):
                        h["feats"] = runner.encode(h["points"], h["n_pts"])
                for h in halves:
                    h["g_dec"] = torch.cuda.CUDAGraph()
                    gathered = h["xbuf"] if use_dist else h["feats"][L]
                    with torch.cuda.graph(h["g_dec"], **h["cap"]):
                        h["out"] = runner.decode(h["feats"], gathered, h["trans"], h["plan"])

            def run():
                cur = torch.cuda.current_stream()
                works = []
                ev = None
                for hi, h in enumerate(halves):     # encoder A, exchange A (async), encoder B, exchange B: the same host order on every rank
                    if two and not free_run:
                        h["stream"].wait_stream(cur)
                    with torch.cuda.stream(h["stream"]):
                        if ev is not None:          # (stagger, first step after an arm only) half B waits for half A's encoder
                            h["stream"].wait_event(ev)
                        h["g_enc"].replay()
                        if self._stagger_armed and hi == 0:
                            ev = torch.cuda.Event()
                            ev.record(h["stream"])
                        works.append(runner.start_exchange(h["feats"][L], out=h["xbuf"])[1] if use_dist else None)
                self._stagger_armed = False
                for h, w in zip(halves, works):
                    with torch.cuda.stream(h["stream"]):
                        self.timed_wait(w)
                        h["g_dec"].replay()
                if two and not free_run:
                    for h in halves:
                        cur.wait_stream(h["stream"])
            self.run = run
            self.exec_mode = ("4 hipGraph segments per step (encoder A, encoder B, fusion+decoder+heads A, B); exchange between them; "
                              + (("the two half-batches on two FREE-RUNNING streams (no join between steps; experiment)" + (", half B one encoder behind half A" if stagger else ""))
                                 if free_run else "the two half-batches on two streams, joined at the end of the step" if two else "one stream"))
        elif mode == 0:
            def run():
                self.last_out = self.step()
            self.run = run
            self.exec_mode = "eager launches"
        else:
            self.run = lambda: None     # a rank without items (agent-per-gpu, rank >= 5): barriers and timing only
            self.exec_mode = "idle rank"

    def outputs(self):
        """Logits of the last step, per half-batch (this rank's items)."""
        if self.mode in (1, 4, 5):
            return [h["out"] for h in self.halves]
        return list(self.last_out)

    def check_sharding(self, n_frames=8):
        """R-rank == 1-rank ON THE GPUS (SURVEY 8e's oracle; also at N = 1, where it checks that a map's bits do not depend on the batch it rides in):
        this rank regenerates, from the seeds, the sweeps of ALL five agents for `n_frames` of the frames it owns items of in half-batch 0, runs
        them through an UNSHARDED 1-rank runner (its own encoder for every agent, no exchange), and compares the logits of its own (agent, frame)
        items bit for bit with what the timed, sharded step produced from the exchanged maps.  -> True / False (None on an idle rank)."""
        from v2x_sim_amd.parallel import AgentShard, ShardedV2VNet
        from v2x_sim_amd.utils.synthetic import synthetic_points
        if not self.active:
            return None
        sh, Bh, h0 = self.shard, self.Bh, self.halves[0]
        frames, pairs = shard_check_plan(sh.rows, Bh, n_frames)
        n_frames = len(frames)
        one = AgentShard(AGENTS, n_frames, 0, 1)
        pts = np.concatenate([synthetic_points(1, POINTS_PER_SWEEP, seed=self.point_seed(0, a * Bh + frames[k])) for a, k in one.items])
        pts = torch.from_numpy(pts).to(self.dev)
        n_pts = torch.full((one.per_rank,), POINTS_PER_SWEEP, dtype=torch.int32, device=self.dev)
        trans = h0["trans"][torch.tensor(frames, device=self.dev)].contiguous()
        plan = one.fusion_plan(torch.full((n_frames, AGENTS), AGENTS), self.dev)
        with torch.no_grad():
            ref = ShardedV2VNet(self.model, one).forward_points(pts, n_pts, trans, plan)
        got = self.outputs()[0]
        ri = torch.tensor([p[0] for p in pairs], device=self.dev)
        gi = torch.tensor([p[1] for p in pairs], device=self.dev)
        ok = all(torch.equal(ref[k].reshape(one.per_rank, -1)[ri], got[k].reshape(sh.per_rank, -1)[gi]) for k in ("cls", "loc"))
        torch.cuda.synchronize()
        return bool(ok)

    def measure(self):
        args, dev = self.args, self.dev
        self.build()
        if not self.capture:
            return None
        for _ in range(2):
            self.run()
        torch.cuda.synchronize()
        self.wait_events.clear()

        self.barrier()
        _mark(MARK_FIRST)       # warm-up, capture and two replayed steps are behind EVERY rank (supervise() stops its stall timer here)
        torch.cuda.synchronize()
        if self.mode == 5 and os.environ.get("V2X_BENCH_STAGGER", "0") == "1":
            self._stagger_armed = True      # the synchronize above re-aligned the streams: the stagger is re-established INSIDE the timed region (its cost is in the number)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            self.run()
        torch.cuda.synchronize()
        self.barrier()
        elapsed = time.perf_counter() - t0
        graph_equals_eager = None           # checked at N = 1 in the graph modes of a --full run
        if args.full and self.mode in (1, 4, 5) and self.active and not self.use_dist:
            # the graphs' outputs (the last replay; the two halves ran concurrently in mode 1) against an eager, one-stream recomputation of the same
            # step: every kernel is deterministic and the halves are independent, so the logits must agree bit for bit
            ref = self.step()
            torch.cuda.synchronize()
            graph_equals_eager = all(torch.equal(h["out"][k], r[k]) for h, r in zip(self.halves, ref) for k in ("cls", "loc"))
            if not graph_equals_eager:      # reported in the record (never silently): the measurement above is of a step whose results are in doubt
                print("bench.py: WARNING: the hipGraph step's logits differ from the eager step's", file=sys.stderr, flush=True)
            del ref
        # sharded == unsharded, on every rank, on what the timed step left in its output buffers
        ok = self.check_sharding() if not args.no_shard_check else None
        okt = torch.tensor([1 if ok in (True, None) else 0], dtype=torch.int32, device=dev)
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        if self.use_dist:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dist.all_reduce(okt, op=dist.ReduceOp.MIN)
        sharded_equals_unsharded = None if args.no_shard_check else bool(int(okt.item()))
        if sharded_equals_unsharded is False:
            print("bench.py: WARNING: a rank's sharded logits differ from its unsharded recomputation", file=sys.stderr, flush=True)
        elapsed = float(t.item())
        # exposed exchange time per step on every rank (0 when the collective finished under the other half's compute)
        exposed = sum(e0.elapsed_time(e1) for e0, e1 in self.wait_events) / max(args.steps, 1)
        self.wait_events.clear()
        exposed_all = [exposed]
        if self.use_dist:
            ex = torch.tensor([exposed], dtype=torch.float64, device=dev)
            gl = [torch.zeros_like(ex) for _ in range(self.world)]
            dist.all_gather(gl, ex)
            exposed_all = [float(x) for x in gl]
        return {"fps": self.Bt * args.steps / elapsed, "ms_per_step": elapsed / args.steps * 1e3, "graph_equals_eager": graph_equals_eager,
                "sharded_equals_unsharded": sharded_equals_unsharded, "exposed_all": exposed_all,
                "ranks_seen": dist.get_world_size() if self.use_dist else 1}


def main():
    argv = sys.argv[1:]
    args = parse(argv)
    launched = "WORLD_SIZE" in os.environ
    if args.gpus > 1 and not args.dry_run:
        # a clear answer instead of "HIP error: invalid device ordinal" out of rank N-1 (device_count does not initialise the GPU on this image)
        have = torch.cuda.device_count()
        if have < args.gpus:
            print("bench.py: --gpus %d requested, this node exposes %d GPU%s" % (args.gpus, have, "" if have == 1 else "s"), file=sys.stderr)
            sys.exit(2)
    if args.gpus > 1 and not launched:
        sys.exit(launch_ranks(args, argv))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("WORLD_SIZE=%d but --gpus %d" % (world, args.gpus))
    if args.frames_per_gpu % 2:
        raise SystemExit("--frames-per-gpu must be even (the step runs as two half-batches)")
    if args.layout == "agent-per-gpu" and world < AGENTS:
        raise SystemExit("--layout agent-per-gpu needs --gpus >= %d (one GPU per agent)" % AGENTS)
    if world > 1 and os.environ.get("V2X_BENCH_CHILD") != "1" and os.environ.get("V2X_BENCH_WATCHDOG", "1") != "0":
        sys.exit(supervise(args, argv, rank, world))      # this process never touches the GPU: the rank runs as its child (see supervise)
    if os.environ.get("V2X_BENCH_CHILD") == "1":
        try:    # Linux: SIGKILL this rank when its supervisor dies, however that happens (prctl PR_SET_PDEATHSIG = 1)
            import ctypes
            ctypes.CDLL(None).prctl(1, 9, 0, 0, 0)
            if os.getppid() == 1:
                sys.exit(125)
        except Exception:
            pass
    if args.dry_run:
        sys.exit(dry_run(args, world, rank))
    if os.environ.get("V2X_BENCH_INNER") == "1" and os.environ.get("V2X_BENCH_FAKE_RECORD"):
        # test hook (tests/test_bench_launcher_cpu.py): the benchmark child of the N = 1 orchestrator replaced by a canned record, so that the parent's
        # relay / counter passes / merge can be exercised on a box without a GPU
        with open(os.environ["V2X_BENCH_FAKE_RECORD"]) as fh:
            print(fh.read().strip(), flush=True)
        sys.exit(0)
    global LIVE_TRAFFIC
    pmc_when = "before the timed run (V2X_BENCH_PMC_ORDER=before: round 5's order, kept for the paired comparison)"
    have_gpu = torch.cuda.device_count() > 0 or os.environ.get("V2X_BENCH_FORCE_ORCHESTRATE") == "1"     # (the second: the CPU test of the orchestrator)
    if world == 1 and args.scaling == "weak" and have_gpu and os.environ.get("V2X_BENCH_INNER") != "1":
        if os.environ.get("V2X_BENCH_PMC_ORDER", "after") == "before":
            LIVE_TRAFFIC = live_traffic_table(args)   # two short child runs under rocprofv3 --pmc, BEFORE this process initialises the GPU
        elif live_traffic_wanted(args)[0]:
            sys.exit(orchestrate(args, argv))         # this process stays off the GPU: the bench runs as a child FIRST, the counter passes after it
        else:
            LIVE_TRAFFIC = (None, live_traffic_wanted(args)[1], 0.0)
    elif os.environ.get("V2X_BENCH_INNER") == "1":
        LIVE_TRAFFIC = (None, "deferred to the parent process (after the timed run)", 0.0)
    if not torch.cuda.is_available():
        print("bench.py needs the MI355X: the product path has no CPU fallback (use --dry-run for the launcher walk)",
              file=sys.stderr)
        sys.exit(3)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # V2X_FORCE_DIST=1: exercise the RCCL code path (process group, bf16 all-gather, barrier, all-reduce) even with
    # one rank -- the only way to smoke-test it on a 1-GPU box
    force_dist = os.environ.get("V2X_FORCE_DIST") == "1"
    use_dist = world > 1 or force_dist
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29531")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    from v2x_sim_amd import ops
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.models.det import V2VNet
    from v2x_sim_amd.utils.synthetic import init_synthetic_weights

    # layout of the (agent, frame) items over the ranks: all of them (spread) or one agent per rank on ranks 0..4 (agent-per-gpu)
    sworld, srank, sgroup = shard_layout(args, world, rank) if use_dist else (1, 0, None)
    active = srank is not None
    model = init_synthetic_weights(V2VNet(Config("test"), gnn_iter_times=args.gnn_iters, num_agent=AGENTS), seed=0)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(dev)
    if active:
        model.packed(dev)
    ctx = dict(args=args, dev=dev, world=world, use_dist=use_dist, force_dist=force_dist, sworld=sworld, srank=srank, sgroup=sgroup,
               active=active, model=model)
    _mark(MARK_READY)       # (supervised N > 1 runs: model, data generator and process group are up; what follows has collectives in it)
    # weak scaling (the headline, per-GPU work fixed): frames = frames_per_gpu * ranks; strong scaling (total work fixed): frames = frames_per_gpu
    # whatever N.  `--scaling weak` (default) times the weak workload and, when N > 1 in a --full run, the strong one as well (sub-record `strong`).
    if args.scaling == "strong":
        if (args.frames_per_gpu // 2 * AGENTS) % sworld:
            raise SystemExit("--scaling strong: %d items per half-batch do not divide over %d ranks" % (args.frames_per_gpu // 2 * AGENTS, sworld))
        wl = Workload(ctx, args.frames_per_gpu)
    else:
        wl = Workload(ctx, args.frames_per_gpu * sworld)
    res = wl.measure()
    if args.dump_outputs and rank == 0 and active:
        dump_outputs(wl.outputs(), args.dump_outputs)
    Bt, fps, ms_per_step, exec_mode, mode = wl.Bt, res["fps"], res["ms_per_step"], wl.exec_mode, wl.mode
    graph_equals_eager, sharded_equals_unsharded = res["graph_equals_eager"], res["sharded_equals_unsharded"]
    exposed_all, ranks_seen = res["exposed_all"], res["ranks_seen"]
    step, halves = wl.step, wl.halves
    strong = None
    if args.full and args.scaling == "weak" and world > 1 and (args.frames_per_gpu // 2 * AGENTS) % sworld == 0:
        wl.release()
        ws = Workload(ctx, args.frames_per_gpu)
        rs = ws.measure()
        strong = {"scaling": "strong", "frames_per_step": ws.Bt, "value": rs["fps"], "unit": "frames/s", "ms_per_step": rs["ms_per_step"],
                  "items_per_rank_and_half_batch": ws.shard.per_rank, "sharded_equals_unsharded": rs["sharded_equals_unsharded"],
                  "exposed_exchange_ms_per_step": rs["exposed_all"],
                  "note": "total work fixed at --frames-per-gpu frames per step whatever N (the weak line keeps per-GPU work fixed)"}
        ws.release()
        wl = Workload(ctx, args.frames_per_gpu * sworld, capture=False)     # the weak workload again: eager steps for the instrumented roofline pass below
        step, halves = wl.step, wl.halves
        if active:
            step()
            torch.cuda.synchronize()

    roofline = None
    kernels = None
    executed_gflop_measured = None
    if not args.no_roofline and active:
        # instrumented pass: HIP events around every launch, on the launch stream (eager, not the graph)
        ops.PROFILE = []
        n_inst = 3
        for _ in range(n_inst):
            step()
        torch.cuda.synchronize()
        recs, ops.PROFILE = ops.PROFILE, None
        groups = {}
        for name, fl, by, e0, e1, _layer in recs:
            gdict = groups.setdefault(name, {"ms": 0.0, "flops": 0.0, "bytes": 0.0, "launches": 0})
            gdict["ms"] += e0.elapsed_time(e1)
            gdict["flops"] += fl
            gdict["bytes"] += by
            gdict["launches"] += 1
        total_ms = sum(v["ms"] for v in groups.values())
        # FLOPs the launches of one step EXECUTE, as each wrapper booked them (a parity-class layer its 4-tap count, a 9-tap layer its 9-tap count:
        # whatever was actually dispatched -- ADVICE r5: not a static table keyed on the PARITY_CLASS switch)
        executed_gflop_measured = sum(v["flops"] for v in groups.values()) / n_inst / 1e9 / (wl.Bt / max(sworld, 1))
        dom = max(groups, key=lambda k: groups[k]["ms"])
        d = groups[dom]
        ai = d["flops"] / max(d["bytes"], 1.0)
        if ai >= PEAK_MFMA_TFLOPS * 1e12 / (PEAK_HBM_GBS * 1e9):
            achieved = d["flops"] / (d["ms"] * 1e-3) / 1e12
            roofline = {"bound": "mfma", "achieved": achieved, "peak": PEAK_MFMA_TFLOPS, "unit": "TFLOP/s",
                        "frac": achieved / PEAK_MFMA_TFLOPS, "traffic": None}
        else:
            achieved = d["bytes"] / (d["ms"] * 1e-3) / 1e9
            roofline = {"bound": "hbm", "achieved": achieved, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                        "frac": achieved / PEAK_HBM_GBS, "traffic": None}
        # HBM traffic per launch of that kernel from the committed PMC passes (rocprofv3 --pmc FETCH_SIZE /
        # WRITE_SIZE, gfx950-corrected by tools/pmc_traffic.py); valid for the default workload (128 frames/GPU) only
        roofline["traffic_source"] = None
        for tname in TRAFFIC_FILES:
            tfile = os.path.join(ROOT, "profiles", tname)
            if os.path.exists(tfile) and args.frames_per_gpu == 128 and args.scaling == "weak":  # 2 half-batches of 64 = the profiled launches
                with open(tfile) as fh:
                    tks = json.load(fh)["kernels"]
                    # (round-3 files name stream8g with its removed fourth template argument)
                    tk = tks.get(dom) or tks.get(dom.replace(", true>", ", true, false>").replace(", false>", ", false, false>"))
                if tk:
                    ff = FETCH_FACTOR.get(dom, FETCH_FACTOR_DEFAULT)     # (summaries older than round 6 hold FETCH_SIZE x 2: rescaled to the kernel's calibrated factor)
                    raw = tk.get("fetch_size_raw_bytes_per_launch", tk["hbm_read_bytes_per_launch"] / 2.0)
                    roofline["traffic"] = raw * ff + tk["hbm_write_bytes_per_launch"]
                    roofline["traffic_source"] = "profiles/%s (committed rocprofv3 --pmc passes of this workload; not re-measured in this run)" % tname
                    break
        roofline["kernel"] = dom
        apply_live_traffic(roofline, LIVE_TRAFFIC, pmc_when)    # (the orchestrating parent overwrites this with its own passes, run AFTER this child)
        roofline.update({"kernel": dom, "avg_launch_us": d["ms"] * 1e3 / d["launches"],
                         "launches_per_step": d["launches"] // n_inst,
                         "share_of_kernel_time": d["ms"] / total_ms,
                         "alg_flops_per_launch": d["flops"] / d["launches"],
                         "alg_bytes_per_launch": d["bytes"] / d["launches"],
                         "timing": "HIP events around every launch of a separate EAGER pass of the same step (not the timed "
                                   "graph replay; the per-kernel sum therefore exceeds ms_per_step by the event overhead)"})
        kernels = {k: {"us_per_step": v["ms"] * 1e3 / n_inst, "launches_per_step": v["launches"] // n_inst,
                       "tflops": v["flops"] / max(v["ms"], 1e-9) / 1e9, "gbs": v["bytes"] / max(v["ms"], 1e-9) / 1e6}
                   for k, v in sorted(groups.items(), key=lambda kv: -kv[1]["ms"])}

    # what THIS box sustains (v2x_calib_stream / v2x_calib_mfma, ~0.3 s): a streaming kernel at the read : write mixes of the HBM-bound layers and
    # a register-resident MFMA loop on random operands, with the shader clock it held -- lets fractions and rounds be compared box-free
    calibration = None
    if rank == 0 and active and not args.no_calibration:
        try:
            from v2x_sim_amd.calibrate import calibrate
            calibration = calibrate(dev)
            if roofline is not None:
                ceil = calibration["mfma_tflops"] if roofline["bound"] == "mfma" else 1e3 * min(calibration["copy_1_1_tbs"], calibration["copy_1_3_tbs"])
                roofline["frac_of_measured_ceiling"] = roofline["achieved"] / ceil
        except Exception as e:      # the headline record must not die with a side table
            calibration = {"error": repr(e)}

    latency = configs = training = host_streaming = None
    if rank == 0 and world == 1 and not args.no_extras and not force_dist:
        # free the step's graphs and buffers first: the extras build their own
        wl.release()
        latency = measure_latency(model, dev)
        latency["default_dispatch"] = measure_latency(model, dev, small_batch=False)
        try:
            import importlib.util
            spec = importlib.util.spec_from_file_location("bench_configs", os.path.join(ROOT, "tools", "bench_configs.py"))
            bc = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(bc)
            configs = bc.run_configs(64, 5, dev)
        except Exception as e:  # the headline record must not die with a side table
            configs = {"error": repr(e)}
        try:
            torch.cuda.empty_cache()
            training = bc.run_training(dev)
        except Exception as e:
            training = {"error": repr(e)}
        try:
            # PCIe-inclusive rate (never `value`): the same 64-frame step fed from pinned host memory, copied inside the step or prefetched on a copy stream
            torch.cuda.empty_cache()
            spec = importlib.util.spec_from_file_location("stream_points", os.path.join(ROOT, "tools", "stream_points.py"))
            sp = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(sp)
            hs, _ = sp.main(64, 8)
            host_streaming = {"frames_per_step": 64, "resident_frames_per_s": hs["resident"], "inline_copy_frames_per_s": hs["inline"],
                              "prefetched_frames_per_s": hs["prefetch"], "prefetched_over_resident": hs["prefetch"] / hs["resident"]}
        except Exception as e:
            host_streaming = {"error": repr(e)}

    cpu = gpu_stock = None
    if rank == 0 and world == 1 and not args.no_gpu_baseline and not force_dist:
        try:
            wl.release()
            gpu_stock = gpu_stock_baseline(state, args.gnn_iters, dev)
        except Exception as e:      # noqa: BLE001
            gpu_stock = {"error": repr(e)[:300]}
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline(state, args.gnn_iters)
        if gpu_stock is not None:   # (the driver's parsed record keeps `cpu_baseline` whole: the same-node GPU comparator rides in it as well)
            cpu["same_node_gpu_stock_baseline"] = {k: gpu_stock.get(k) for k in ("fp32_frames_per_s", "bf16_autocast_channels_last_frames_per_s", "frames", "what")}

    from v2x_sim_amd import tuning as _tuning
    parity_saved = GFLOP_PARITY_CLASS_SAVED[max(0, min(3, _tuning.get("PARITY_CLASS")))]
    reference_gflop = GFLOP_PER_FRAME_BASE + GFLOP_PER_GNN_ROUND * args.gnn_iters
    # executed FLOPs per frame: what the instrumented pass's launches booked (falls back to the static table without that pass)
    executed_gflop = executed_gflop_measured if executed_gflop_measured else reference_gflop - parity_saved
    if rank == 0 and isinstance(training, dict):
        training["frac_of_mfma_peak"] = training_fractions(training)
        # the step's HBM side: bytes per step from the committed rocprofv3 --pmc passes (tools/train_step_profile.sh -> tools/train_traffic_table.py), priced at
        # THIS run's step time -- the training step is memory-side (batch-statistics BatchNorm is 8 passes over every convolution's output), which is why its
        # MFMA fraction is low; both fractions are reported
        training["hbm"] = {}
        for maps, key in ((10, "FaFNet_10_maps"), (40, "FaFNet_40_maps")):
            tf = os.path.join(ROOT, "profiles", "r06_train_traffic_%d.json" % maps)
            try:
                with open(tf) as fh:
                    tj = json.load(fh)
                nbytes = tj["hbm_read_bytes_per_step"] + tj["hbm_write_bytes_per_step"]
                ms = 3.0 * TRAIN_FWD_GFLOP_PER_MAP["FaFNet"] * maps / (training["frac_of_mfma_peak"][key] * PEAK_MFMA_TFLOPS)
                training["hbm"][key] = {"bytes_per_step": nbytes, "source": "profiles/r06_train_traffic_%d.json (committed PMC passes)" % maps,
                                        "tb_s": nbytes / ms / 1e9, "frac_of_8_tb_s": nbytes / ms / 1e9 / (PEAK_HBM_GBS / 1e3)}
            except Exception as e:      # noqa: BLE001
                training["hbm"][key] = {"error": repr(e)[:200]}
    if rank == 0:
        summary = build_summary(fps, ms_per_step, latency, configs, training, gpu_stock, cpu, roofline, executed_gflop, world)
        # the N > 1 self-checks as scalars too: a first SCALE run keeps them whatever the driver's parser drops
        summary.update({"n_gpus": world, "ranks_seen": ranks_seen, "sharded_equals_unsharded": sharded_equals_unsharded,
                        "exposed_exchange_ms_per_step_max": max(exposed_all) if exposed_all else None})
        if strong is not None:
            summary.update({"strong_frames_per_s": strong["value"], "strong_ms_per_step": strong["ms_per_step"],
                            "strong_sharded_equals_unsharded": strong["sharded_equals_unsharded"],
                            "strong_exposed_exchange_ms_per_step_max": max(strong["exposed_exchange_ms_per_step"]) if strong["exposed_exchange_ms_per_step"] else None})
        rec = {
            "metric": "BEV frames/sec, V2VNet 5-agent detection (256x256 BEV)", "value": fps, "unit": "frames/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step,
            "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None, "dtype": "bf16", "full": args.full,
            "data": "synthetic (seeded 65536-pt sweeps per agent, random SE(2) poses, He-init weights)",
            "config": {"workload": "V2VNet 5-agent detection, points->logits (a1-a7), gnn_iter=%d" % args.gnn_iters,
                       "agents": AGENTS, "frames_per_step": Bt, "frames_per_gpu": Bt // max(sworld, 1),
                       "layout": args.layout, "active_ranks": sworld,
                       "half_batches": 2,
                       "points_per_agent": POINTS_PER_SWEEP, "bev": [256, 256, 13],
                       "sharding": ("agent-major (agent,frame) items, contiguous slices; async RCCL %s of the fusion "
                                    "maps of one half-batch overlapped with the other half's compute"
                                    % ("all-gather" if args.transport == "allgather" else "grouped send/recv of the needed rows"))
                                   if world > 1 else "single GPU, no collective",
                       "exec_mode": exec_mode, "hip_graph": bool(mode)},
            # fraction of the bf16 MFMA peak from the FLOPs the kernels EXECUTE: conv8_1, conv5_1 and conv6_1 run in the parity-class form (4 instead of
            # 9 taps on their x2-upsampled source, -6.7 GFLOP per frame each; tuning switch PARITY_CLASS); the reference's 9-tap count is quoted beside it
            "whole_step_frac": executed_gflop * 1e9 * fps / world / (PEAK_MFMA_TFLOPS * 1e12),
            "executed_gflop_per_frame": executed_gflop,
            "executed_gflop_source": "sum of the FLOPs booked by the launches of the instrumented pass" if executed_gflop_measured else "static table (no instrumented pass)",
            "reference_gflop_per_frame": reference_gflop,
            "whole_step_frac_at_reference_flops": reference_gflop * 1e9 * fps / world / (PEAK_MFMA_TFLOPS * 1e12),
            "launch": launch_record(args),
            "graph_equals_eager": graph_equals_eager,
            "sharded_equals_unsharded": sharded_equals_unsharded,
            "sharded_equals_unsharded_note": "every rank recomputes 8 frames of half-batch 0 UNSHARDED (all five agents' sweeps regenerated from their seeds, its own "
                                             "encoder, no exchange) and compares the logits of its own items bit for bit with the timed sharded step's; min over ranks",
            "strong": strong,
            "ranks_seen": ranks_seen, "exposed_exchange_ms_per_step": exposed_all,
            "exposed_exchange_note": "HIP-event time a half-batch's stream waits for its exchange; with the two half-batches on two streams the GPU runs "
                                     "the other half's kernels during that wait (one-stream order: --graph 4)",
            "kernels": kernels, "hbm_side_kernels_vs_stream_ceiling": stream_ceiling_fractions(kernels, calibration), "roofline": roofline, "calibration": calibration, "cpu_baseline": cpu, "gpu_stock_baseline": gpu_stock, "latency": latency, "configs": configs,
            "training": training, "host_streaming": host_streaming,
        }
        # top-level scalars the driver's parser can keep (BASELINE.md section 3's batch sizes, the five configs, the N > 1 self-checks), then the
        # compact `summary` as the LAST key of the line (the driver stores the tail of stdout)
        rec.update({k: v for k, v in summary.items() if not isinstance(v, (dict, list)) and k not in rec})
        rec["summary"] = summary
    if use_dist:
        dist.destroy_process_group()
    # RCCL prints its version banner through C stdio, which (on a pipe) is only flushed at exit and would land
    # AFTER our JSON line: flush C stdio first so that the JSON record is the last line of stdout.
    try:
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    if rank == 0:
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
