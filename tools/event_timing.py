"""What tools/time_fps.py, time_group.py and time_propagate.py share: HIP-event timing of a callable, the median of the rounds, and
the first line and the writing of their reports."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(torch, fn, inner):
    """ms per call: events around `inner` back-to-back calls, then a synchronise."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        res = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner, res


def median(v):
    return sorted(v)[len(v) // 2]


def header(torch):
    """The report's first line: commit, GPU, torch."""
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                                text=True).stdout.strip()
    except OSError:
        commit = ""
    return "commit %s   GPU %s   torch %s" % (commit or "(not a git checkout)", torch.cuda.get_device_name(0), torch.__version__)


def emit(lines, out):
    """Print the report and, with --out, write it there."""
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)
