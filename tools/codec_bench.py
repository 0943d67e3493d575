#!/usr/bin/env python3
"""Time of the fused codec kernel (csrc/codec.hip) at the bench geometry, M = 640 * 1024 pixels of C = 256 channels, for compress_level k in
{1, 2, 4, 8}, against (a) the same two layers as two v2x_conv2d 1x1 launches of the existing kernels and (b) this box's 1:1 streaming
ceiling (v2x_calib_stream).  The two forms ALTERNATE inside one process (fused, two-launch, fused, ...), medians over the rounds.

    python3 tools/codec_bench.py [--rounds 30] [--out profiles/codec_kernel.txt]

The two-launch form carries a message of < 8 channels padded to 8 (the gather kernel's channel quantum); its intermediate makes an HBM
round trip, which the fused form does not."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "v2x-sim_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", default=30, type=int)
    ap.add_argument("--maps", default=640, type=int, help="32 x 32 maps per launch")
    ap.add_argument("--out", default="", type=str)
    args = ap.parse_args(argv)
    from v2x_sim_amd import calibrate, ops, packing
    dev = torch.device("cuda:0")
    C, M = 256, args.maps * 1024
    g = torch.Generator().manual_seed(0)
    x = torch.relu(torch.randn(args.maps, 32, 32, C, generator=g)).to(torch.bfloat16).to(dev)
    ceiling = max(calibrate.stream_rate(1, 1, 2 << 30, False, wg, 2, dev) for wg in (2, 4, 8))
    lines = ["codec kernel, M = %d x 1024 pixels, C = %d, bf16; medians of %d alternating rounds; 1:1 streaming ceiling of this box %.2f TB/s"
             % (args.maps, C, args.rounds, ceiling),
             "bytes = 2 C in + 2 C out per pixel (the fused form's whole traffic; the message stays on chip)",
             "%-3s %-4s %10s %10s %10s %12s %12s" % ("k", "Cc", "fused us", "TB/s", "2-launch us", "fused/2-launch", "of ceiling")]
    for k in (1, 2, 4, 8):
        Cc = C >> k
        torch.manual_seed(k)
        conv_c, bn_c = torch.nn.Conv2d(C, Cc, 1), torch.nn.BatchNorm2d(Cc).eval()
        conv_d, bn_d = torch.nn.Conv2d(Cc, C, 1), torch.nn.BatchNorm2d(C).eval()
        pc = packing.pack_codec("codec", conv_c, bn_c, conv_d, bn_d, device=dev)
        # the two-launch form: gather-layout 1x1 layers (the streaming 1x1 kernel takes them where Cin, Cout <= 128, the gather kernel otherwise)
        cp = max(Cc, 8)
        s1, t1 = packing.fold_bn(conv_c.bias, bn_c, Cc)
        s2, t2 = packing.fold_bn(conv_d.bias, bn_d, C)
        w1 = torch.zeros(cp, C, 1, 1)
        w1[:Cc] = conv_c.weight.detach()
        w2 = torch.zeros(C, cp, 1, 1)
        w2[:, :Cc] = conv_d.weight.detach()
        p1 = packing.pack_conv("compress", w1, torch.cat([s1, torch.ones(cp - Cc)]), torch.cat([t1, torch.zeros(cp - Cc)]), stride=1, pad=0, device=dev)
        p2 = packing.pack_conv("decompress", w2, s2, t2, stride=1, pad=0, device=dev)
        fused = lambda: ops.codec(pc, x)                               # noqa: E731
        two = lambda: ops.conv2d(p2, ops.conv2d(p1, x))                # noqa: E731
        ya, yb = fused(), two()
        same = bool(torch.equal(ya, yb))
        for _ in range(3):
            fused()
            two()
        torch.cuda.synchronize()
        tf, tt = [], []
        for _ in range(args.rounds):
            tf.append(_timed(fused))
            tt.append(_timed(two))
        f, t = float(np.median(tf)), float(np.median(tt))
        rate = 4.0 * C * M / f / 1e6
        lines.append("%-3d %-4d %10.1f %10.2f %10.1f %12.3f %12.3f   (same bits as the two launches: %s)" % (k, Cc, f, rate, t, f / t, rate / ceiling, same))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
