"""Step state for graph replay: a device int32 counter that is tied to ``global_step``, and its host side.

The protocol: before the launch that reads it, the device counter equals ``global_step.value`` (with no global step it
free-runs); a host mirror says what the device holds; an eager call that finds the two different (``global_step.assign``, a
restored checkpoint) uploads the value; a call under stream capture raises instead, because a captured upload would replay a
frozen value; a graph replay moves the mirror by +1; a capture, which enqueues nothing, is undone with -1.  train.GraphedStep
keeps it for the participants the optimizer names (``step_participants``) through ``fresh`` and ``moved``.  Free-running
counters (dropout's, DeviceCifar's, Adam's beta powers) have no mirror and are no StepCounters.
"""
import torch


def int32(v):
  """v as a device int32 holds it (two's-complement wrap-around)."""
  return (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31


class StepCounter:
  """``tensor``: int32 [1] on ``device``, read and advanced by a kernel; ``mirror``: what it holds; ``what``: its name in errors."""

  def __init__(self, device, what):
    self.tensor = torch.zeros(1, dtype=torch.int32, device=device)
    self.mirror = 0
    self.what = what

  def fresh(self, global_step):
    return int32(global_step.value) == self.mirror

  def sync(self, global_step):
    """In front of the launch that reads the counter: uploads ``global_step.value`` where the mirror says otherwise."""
    if global_step is None or self.fresh(global_step):
      return
    want = int32(global_step.value)
    if torch.cuda.is_current_stream_capturing():
      raise RuntimeError('the %s device step counter (%d) differs from global_step (%d) during graph capture: run one eager '
                         'step after changing global_step' % (self.what, self.mirror, want))
    self.tensor.fill_(want)
    self.mirror = want

  def moved(self, k):
    """The device counter moved by ``k``: +1 a launch or a graph replay, -1 undoing the host side of a capture."""
    self.mirror = int32(self.mirror + k)
