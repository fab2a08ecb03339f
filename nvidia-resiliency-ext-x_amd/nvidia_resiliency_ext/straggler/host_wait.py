"""How the host waits for a report's results (they land in pinned host memory):
  "bounded" (default) -- poll the completion event for at most SPIN_BOUND_US, then block in
      hipEventSynchronize on a blocking-sync event: a report that lands within the bound skips
      the driver's wake-up latency, a longer one does not hold a host core (in a training process
      every core belongs to the job; the reference's report path blocks too, straggler.py:234-235);
  "spin" -- poll until done (bench.py: the wake-up latency is part of every timed report);
  "block" -- block at once.
NVRX_SYNC selects the mode per process; set_sync_mode() changes it at run time."""
import os
import time
from typing import Optional

import torch

SYNC_MODES = ("bounded", "spin", "block")
SPIN_BOUND_US = float(os.environ.get("NVRX_SPIN_US", "50"))
_sync_mode = os.environ.get("NVRX_SYNC", "") or "bounded"
if _sync_mode not in SYNC_MODES:
    raise ValueError(f"NVRX_SYNC={_sync_mode!r}: one of {SYNC_MODES}")


def set_sync_mode(mode: str) -> str:
    """Select how report results are waited for (SYNC_MODES); returns the previous mode."""
    global _sync_mode
    if mode not in SYNC_MODES:
        raise ValueError(f"sync mode {mode!r}: one of {SYNC_MODES}")
    prev, _sync_mode = _sync_mode, mode
    return prev


def sync_mode() -> str:
    return _sync_mode


def wait_event(ev, mode: Optional[str] = None, bound_us: Optional[float] = None) -> None:
    """Wait until a recorded event has completed, in the current (or the given) sync mode.
    `ev` needs query() and synchronize(); the blocking fallback blocks only if the event was
    created with blocking=True (every event the batch API waits on is)."""
    mode = mode or _sync_mode
    if mode == "block":
        ev.synchronize()
        return
    if mode == "spin":
        while not ev.query():
            pass
        return
    bound = SPIN_BOUND_US if bound_us is None else bound_us
    deadline = time.perf_counter_ns() + int(bound * 1e3)
    while not ev.query():
        if time.perf_counter_ns() >= deadline:
            ev.synchronize()
            return


def _wait(device) -> None:
    """Wait for the device's current stream (wait_event on an event recorded on it)."""
    ev = torch.cuda.Event(blocking=True)
    ev.record(torch.cuda.current_stream(device))
    wait_event(ev)
