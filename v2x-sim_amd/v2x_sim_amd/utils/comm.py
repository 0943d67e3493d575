"""The drivers' communication flags (upstream tools/det/train_codet.py / test_codet.py: --compress_level, --only_v2i): parsing, the models'
constructor arguments, and the record kept in / checked against a checkpoint."""


def add_arguments(ap):
    ap.add_argument("--compress_level", default=0, type=int,
                    help="k in 0..8: 1x1 compress / decompress pair around the transmitted 256-channel map; the message has 256 >> k channels")
    ap.add_argument("--only_v2i", default=0, type=int, help="1: vehicles hear the road-side unit (agent 0) only")


def model_kwargs(args, intermediate=True):
    """-> constructor arguments of an intermediate-fusion model; the single-agent baselines exchange nothing and refuse the flags."""
    if not 0 <= args.compress_level <= 8:
        raise SystemExit("--compress_level must be in 0..8")
    if not intermediate:
        if args.compress_level or args.only_v2i:
            raise SystemExit("--compress_level / --only_v2i need a model that exchanges feature maps (not --com %s)" % args.com)
        return {}
    return {"compress_level": int(args.compress_level), "only_v2i": bool(args.only_v2i)}


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

    def __init__(self, compress_level=0, only_v2i=False, late=False):
        self.value = {"compress_level": int(compress_level), "only_v2i": bool(only_v2i)}
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
        kw = {"only_v2i": bool(args.only_v2i), "late": True}
        args.only_v2i = 0                       # the checkpoint is a lowerbound one: it was trained without links
    else:
        kw = model_kwargs(args, intermediate=args.com not in ("lowerbound", "upperbound"))
    if args.resume:
        import torch
        check_checkpoint(torch.load(args.resume, map_location="cpu"), args)
    with model_flags(**(kw or {})) as flags:
        res = driver_main(rest)
    if late:
        st = flags.value["late_stats"]
        print(late_report(st))
        if isinstance(res, dict):
            res["late_kept"], res["late_from_neighbours"] = st["kept"], st["from_neighbours"]
    return res


def late_report(stats):
    """The line the drivers print under --com late; stats = FaFModule.late_stats."""
    egos = max(1, stats["egos"])
    return "late fusion: %d of the %d kept boxes came from neighbours (%.2f of %.2f per ego, %d egos)" % (
        stats["from_neighbours"], stats["kept"], stats["from_neighbours"] / egos, stats["kept"] / egos, stats["egos"])
