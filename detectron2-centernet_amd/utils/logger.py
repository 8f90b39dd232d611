"""`setup_logger` (reference: detectron2/utils/logger.py:27-91, without termcolor): the package's logger writes to stdout on
the main process and to `OUTPUT_DIR/log.txt` -- `log.txt.rankN` on the other ranks -- on every process."""
import functools
import logging
import os
import sys

__all__ = ["setup_logger"]

ROOT_LOGGER = __name__.split(".")[0]      # the package: every module's `logging.getLogger(__name__)` is its child


@functools.lru_cache()
def setup_logger(output=None, distributed_rank=0, *, name=ROOT_LOGGER, abbrev_name=None):
    """output: a directory (-> `log.txt` in it), a `.txt` / `.log` file name, or None for no file.  Returns the logger; a second
    call with the same arguments adds no second handler."""
    logger = logging.getLogger(name)
    logger.setLevel(logging.DEBUG)
    logger.propagate = False
    short = abbrev_name if abbrev_name is not None else name
    plain = logging.Formatter("[%(asctime)s] %(name)s %(levelname)s: %(message)s", datefmt="%m/%d %H:%M:%S")
    if distributed_rank == 0:
        ch = logging.StreamHandler(stream=sys.stdout)
        ch.setLevel(logging.DEBUG)
        ch.setFormatter(logging.Formatter("[%(asctime)s " + short + "]: %(message)s", datefmt="%m/%d %H:%M:%S"))
        logger.addHandler(ch)
    if output:
        filename = output if output.endswith(".txt") or output.endswith(".log") else os.path.join(output, "log.txt")
        if distributed_rank > 0:
            filename = filename + ".rank{}".format(distributed_rank)
        if os.path.dirname(filename):
            os.makedirs(os.path.dirname(filename), exist_ok=True)
        fh = logging.StreamHandler(_cached_log_stream(filename))
        fh.setLevel(logging.DEBUG)
        fh.setFormatter(plain)
        logger.addHandler(fh)
    return logger


@functools.lru_cache(maxsize=None)
def _cached_log_stream(filename):
    return open(filename, "a")
