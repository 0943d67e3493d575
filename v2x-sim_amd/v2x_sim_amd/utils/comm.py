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

    def __init__(self, compress_level=0, only_v2i=False):
        self.value = {"compress_level": int(compress_level), "only_v2i": bool(only_v2i)}

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
    every other argument goes to `driver_main` unchanged.  --com lowerbound / upperbound exchange nothing and refuse the flags."""
    import argparse
    ap = argparse.ArgumentParser(add_help=False)
    add_arguments(ap)
    ap.add_argument("--com", default="v2v", type=str)
    ap.add_argument("--resume", default="", type=str)
    args, rest = ap.parse_known_args(argv)
    rest = list(rest) + ["--com", args.com] + (["--resume", args.resume] if args.resume else [])
    kw = model_kwargs(args, intermediate=args.com not in ("lowerbound", "upperbound"))
    if args.resume:
        import torch
        check_checkpoint(torch.load(args.resume, map_location="cpu"), args)
    with model_flags(**(kw or {})):
        return driver_main(rest)
