"""One rank of a multi-rank run of the command line, as a process of its own (tests/test_gpu_ranks.py starts one per rank):

    python tests/rank_worker.py --rank R --world W --port P --timeout SECONDS [--part-bytes N] -- aio -i in.bam ...

It sets what torchrun would set (RANK, WORLD_SIZE, LOCAL_RANK=0, MASTER_ADDR, MASTER_PORT), AMPLIPY_PART_BYTES when given and
sys.argv to the pinned command line that @PG and ##source record in the command-line tests, initialises torch.distributed with
the GLOO backend -- ranks of which can share one card, which RCCL's cannot -- and calls amplipy.main on the arguments behind
``--``.  parallel.init_from_env leaves an initialised process group alone, so everything behind it is run_amplipy's own
multi-rank path on the real engine.  The exit status is main's; stderr is the log.

The one thing that may differ from a run under RCCL is the all-reduce of a DEVICE tensor.  Where this torch's gloo takes device
tensors, nothing is replaced.  Where it refuses them -- tried once, on a tensor of one word, by every rank alike -- the worker
replaces parallel.allreduce_table, and nothing else, with one that sums a host copy and copies the result back.  Which of the
two ran is the log line "rank_worker: all-reduce of device tensors: ...".

So that a test can tell which rank made which file, every file the interpreter opens for writing is logged too, through an audit
hook ("rank_worker: opens for writing: PATH"; what a C library opens, a rank's own trimmed BAM, is not seen).
"""
import argparse
import datetime
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINNED_ARGV = ["amplipy_amd", "pinned"]
DIRECT, HOST_COPY = "gloo takes them", "gloo refuses them, summed through a host copy"


def allreduce_through_host(dist, table):
    """parallel.allreduce_table for a gloo that takes host tensors only."""
    host = table.cpu()
    dist.all_reduce(host, op=dist.ReduceOp.SUM)
    table.copy_(host)


def log_opens_for_writing(event, args):
    if event == "open" and isinstance(args[0], (str, bytes)) and isinstance(args[2], int) and args[2] & (os.O_WRONLY | os.O_RDWR | os.O_CREAT):
        print("rank_worker: opens for writing: %s" % os.fsdecode(args[0]), file=sys.stderr, flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--world", type=int, required=True)
    ap.add_argument("--port", type=int, required=True)
    ap.add_argument("--timeout", type=float, required=True, help="of every collective, in seconds")
    ap.add_argument("--part-bytes", type=int, default=None)
    ap.add_argument("command", nargs=argparse.REMAINDER)
    a = ap.parse_args(argv)
    command = a.command[1:] if a.command[:1] == ["--"] else a.command
    os.environ.update(RANK=str(a.rank), WORLD_SIZE=str(a.world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(a.port))
    if a.part_bytes is not None:
        os.environ["AMPLIPY_PART_BYTES"] = str(a.part_bytes)
    sys.argv = list(PINNED_ARGV)
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=a.rank, world_size=a.world, timeout=datetime.timedelta(seconds=a.timeout))
    from amplipy_amd import amplipy, parallel
    probe = torch.ones(1, dtype=torch.int32, device="cuda:0")
    try:
        dist.all_reduce(probe, op=dist.ReduceOp.SUM)
        how = DIRECT
    except (RuntimeError, ValueError, NotImplementedError):        # (refused on every rank alike, before anything is sent)
        parallel.allreduce_table = allreduce_through_host
        allreduce_through_host(dist, probe)
        how = HOST_COPY
    assert int(probe.item()) == a.world
    print("rank_worker: all-reduce of device tensors: %s" % how, file=sys.stderr, flush=True)
    sys.addaudithook(log_opens_for_writing)
    return amplipy.main(command)


if __name__ == "__main__":
    sys.exit(main())
