from . import checkpoints, distributed, evaluate, logger, stream, train  # noqa: F401
