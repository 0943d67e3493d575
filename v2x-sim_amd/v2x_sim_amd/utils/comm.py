"""The drivers' communication flags (upstream tools/det/train_codet.py / test_codet.py: --compress_level, --only_v2i): parsing, the models'
constructor arguments, and the record kept in / checked against a checkpoint."""


def add_arguments(ap):
    ap.add_argument("--compress_level", default=0, type=int,
                    help="k in 0..8: 1x1 compress / decompress pair around the transmitted 256-channel map; the message has 256 >> k channels")
    ap.add_argument("--only_v2i", default=0, type=int, help="1: vehicles hear the road-side unit (agent 0) only")
    ap.add_argument("--p_com_outage", default=0.0, type=float,
                    help="evaluation condition: every directed link is down with this probability at every step, drawn on the device (0..1)")
    ap.add_argument("--pose_noise", default=0.0, type=float,
                    help="evaluation condition: sigma in metres of Gaussian noise on the translation of every agent-to-agent transform")
    ap.add_argument("--channel_seed", default=0, type=int, help="seed of the link / pose draws: (seed, step) determines every draw")


def model_kwargs(args, intermediate=True):
    """-> constructor arguments of an intermediate-fusion model; the single-agent baselines exchange nothing and refuse the flags."""
    if not 0 <= args.compress_level <= 8:
        raise SystemExit("--compress_level must be in 0..8")
    if not intermediate:
        if args.compress_level or args.only_v2i:
            raise SystemExit("--compress_level / --only_v2i need a model that exchanges feature maps (not --com %s)" % args.com)
        return {}
    return {"compress_level": int(args.compress_level), "only_v2i": bool(args.only_v2i)}


def channel_kwargs(args, intermediate=True):
    """The degraded-link flags (--p_com_outage, --pose_noise, --channel_seed) -> model_flags() arguments.  An evaluation
    condition, not a property of a checkpoint: never recorded in one, never checked against one.  The single-agent baselines and late fusion
    exchange no feature maps and refuse them."""
    p, sigma = float(getattr(args, "p_com_outage", 0.0)), float(getattr(args, "pose_noise", 0.0))
    if not 0.0 <= p <= 1.0:
        raise SystemExit("--p_com_outage must lie in [0, 1]")
    if not 0.0 <= sigma < float("inf"):
        raise SystemExit("--pose_noise must be finite and >= 0")
    if p == 0.0 and sigma == 0.0:
        return {}
    if not intermediate:
        raise SystemExit("--p_com_outage / --pose_noise need a model that exchanges feature maps (not --com %s)" % args.com)
    return {"p_com_outage": p, "pose_noise": sigma, "channel_seed": int(getattr(args, "channel_seed", 0))}


def refuse_channel_in_training(args):
    """The training drivers share add_arguments(): the degraded-link flags are an evaluation condition and are refused there, not ignored."""
    if getattr(args, "p_com_outage", 0.0) or getattr(args, "pose_noise", 0.0):
        raise SystemExit("--p_com_outage / --pose_noise are evaluation conditions (eval_codet.py, eval_seg.py), not training flags")


def checkpoint_fields(args):
    return {"compress_level": int(args.compress_level), "only_v2i": bool(args.only_v2i)}


def check_checkpoint(ckpt, args):
    """A checkpoint written by the training drivers records both flags: evaluating or resuming it under other flags is refused (a checkpoint
    without the record -- upstream's, or an older one -- is held to its state_dict keys alone)."""
    if not isinstance(ckpt, dict):
        return
    for key, want in checkpoint_fields(args).items():
        if key in ckpt and type(want)(ckpt[key]) != want:
            raise SystemExit("the checkpoint was trained with --%s %s, this run asks for %s" % (key, int(ckpt[key]), int(want)))


_flags = __import__("threading").local()


class model_flags:
    """with comm.model_flags(compress_level=k, only_v2i=v): intermediate-fusion models constructed by THIS thread inside the block, with the
    two arguments left at their defaults, take these values (IntermediateModelBase.__init__ reads them).  For callers that build the model
    somewhere they do not control -- the evaluation drivers, whose files are part of the test surface and stay as they are."""

    def __init__(self, compress_level=0, only_v2i=False, late=False, p_com_outage=0.0, pose_noise=0.0, channel_seed=0):
        self.value = {"compress_level": int(compress_level), "only_v2i": bool(only_v2i)}
        if p_com_outage or pose_noise:
            # the degraded-link condition: the models built inside the block take it and list themselves, so that the
            # evaluation tools can print the realised share of links up
            self.value.update(p_com_outage=float(p_com_outage), pose_noise=float(pose_noise), channel_seed=int(channel_seed), channel_models=[])
        if late:
            # late fusion (--com late): a FaFModule built inside the block exchanges detections; only_v2i is then its link mask, and the module
            # counts into late_stats what its egos kept and how much of it came from neighbours
            self.value.update(late=True, late_stats={"egos": 0, "kept": 0, "from_neighbours": 0})

    def __enter__(self):
        self.prev = getattr(_flags, "value", None)
        _flags.value = self.value
        return self

    def __exit__(self, *exc):
        _flags.value = self.prev
        return False


def current_model_flags():
    return getattr(_flags, "value", None)


def run_eval_driver(driver_main, argv):
    """An evaluation driver's main() (tools/det/test_codet.py, tools/seg/test_seg.py) with the two communication flags: --compress_level /
    --only_v2i are taken out of `argv`, checked against the record in the --resume checkpoint, and given to the model through model_flags();
    every other argument goes to `driver_main` unchanged.  --com lowerbound / upperbound exchange nothing and refuse the flags.
    --p_com_outage / --pose_noise / --channel_seed (degraded links) travel the same way but are an evaluation condition:
    no checkpoint records them; lowerbound / upperbound / late refuse them; the realised share of links up is printed after the metrics.
    --com late (upstream's late fusion) is handled HERE, the driver's own file staying as it is: the driver runs as --com lowerbound (FaFNet, a
    lowerbound checkpoint), the FaFModule it builds reads `late` from model_flags() and fuses the agents' detections (FaFModule.late_fusion);
    --only_v2i is then the link mask of the exchanged boxes (not a property of the checkpoint), --compress_level is refused.  After the run the
    share of the kept boxes that came from neighbours is printed and added to a dict result."""
    import argparse
    ap = argparse.ArgumentParser(add_help=False)
    add_arguments(ap)
    ap.add_argument("--com", default="v2v", type=str)
    ap.add_argument("--resume", default="", type=str)
    args, rest = ap.parse_known_args(argv)
    late = args.com == "late"
    rest = list(rest) + ["--com", "lowerbound" if late else args.com] + (["--resume", args.resume] if args.resume else [])
    if late:
        if args.compress_level:
            raise SystemExit("--compress_level needs a model that exchanges feature maps (not --com late: boxes are exchanged)")
        if args.p_com_outage or args.pose_noise:
            raise SystemExit("--p_com_outage / --pose_noise need a model that exchanges feature maps (not --com late: boxes are exchanged)")
        kw = {"only_v2i": bool(args.only_v2i), "late": True}
        args.only_v2i = 0                       # the checkpoint is a lowerbound one: it was trained without links
    else:
        kw = model_kwargs(args, intermediate=args.com not in ("lowerbound", "upperbound"))
        kw.update(channel_kwargs(args, intermediate=args.com not in ("lowerbound", "upperbound")))
    if args.resume:
        import torch
        check_checkpoint(torch.load(args.resume, map_location="cpu"), args)
    with model_flags(**(kw or {})) as flags:
        res = driver_main(rest)
    if flags.value.get("channel_models"):
        up, possible = (sum(v) for v in zip(*[m.channel_link_stats() for m in flags.value["channel_models"]]))
        print(channel_report(up, possible, flags.value))
        if isinstance(res, dict):
            res["links_up"], res["links_possible"] = up, possible
    if late:
        st = flags.value["late_stats"]
        print(late_report(st))
        if isinstance(res, dict):
            res["late_kept"], res["late_from_neighbours"] = st["kept"], st["from_neighbours"]
    return res


def channel_report(up, possible, flags):
    """The line the evaluation tools print next to their metrics under --p_com_outage / --pose_noise."""
    return "degraded links: %d of the %d links of the static plans were up (share %.4f) at p_com_outage %g, pose_noise %g m, seed %d" % (
        up, possible, up / max(1, possible), flags["p_com_outage"], flags["pose_noise"], flags["channel_seed"])


def late_report(stats):
    """The line the drivers print under --com late; stats = FaFModule.late_stats."""
    egos = max(1, stats["egos"])
    return "late fusion: %d of the %d kept boxes came from neighbours (%.2f of %.2f per ego, %d egos)" % (
        stats["from_neighbours"], stats["kept"], stats["from_neighbours"] / egos, stats["kept"] / egos, stats["egos"])
