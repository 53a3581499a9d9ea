"""CPU checks of rigl_amd.step_state: the int32 wrap, and the whole host protocol of a StepCounter on a CPU tensor -- fresh /
sync with and without a global step, the refusal under stream capture (the capture query is patched: it raises on a machine
with no device), the mirror's moves at the wrap -- and the summaries' pairing of mirror moves with the ring ledger."""
import pytest
import torch

from rigl_amd import summaries
from rigl_amd.step_state import StepCounter, int32


class _GS:
  def __init__(self, value):
    self.value = value


@pytest.fixture
def capturing(monkeypatch):
  """Sets what torch.cuda.is_current_stream_capturing() answers; not capturing until told otherwise."""
  def answer(value):
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: value)
  answer(False)
  return answer


def _state(c):
  return int(c.tensor[0]), c.mirror


def test_int32_wraps_like_the_device():
  assert int32(2 ** 31) == -2 ** 31
  assert int32(-1) == -1
  assert int32(2 ** 32 + 5) == 5
  assert int32(2 ** 31 - 1) == 2 ** 31 - 1 and int32(-2 ** 31) == -2 ** 31 and int32(0) == 0


def test_a_new_counter_is_zero_on_its_device():
  c = StepCounter('cpu', 'test')
  assert c.tensor.dtype == torch.int32 and tuple(c.tensor.shape) == (1,) and c.tensor.device.type == 'cpu'
  assert _state(c) == (0, 0) and c.what == 'test'


def test_sync_without_a_global_step_free_runs(capturing):
  c = StepCounter('cpu', 'test')
  c.moved(3)
  c.sync(None)
  assert _state(c) == (0, 3)                          # nothing uploaded, the mirror is left alone
  capturing(True)
  c.sync(None)                                        # and nothing to refuse under capture
  assert _state(c) == (0, 3)


def test_sync_with_an_equal_global_step_uploads_nothing(capturing):
  c = StepCounter('cpu', 'test')
  c.moved(7)                                          # seven launches advanced the device counter: stand in for them
  c.tensor.fill_(7)
  assert c.fresh(_GS(7)) and not c.fresh(_GS(8))
  c.tensor.fill_(-5)                                  # a sentinel: a fresh sync must not write the tensor
  c.sync(_GS(7))
  assert _state(c) == (-5, 7)
  capturing(True)
  c.sync(_GS(7))                                      # fresh: fine under capture too
  assert _state(c) == (-5, 7)


def test_sync_with_a_different_global_step_uploads_tensor_and_mirror(capturing):
  c = StepCounter('cpu', 'test')
  assert not c.fresh(_GS(41))
  c.sync(_GS(41))
  assert _state(c) == (41, 41) and c.fresh(_GS(41))
  c.sync(_GS(2 ** 31))                                # the global step is a Python int: the counter holds its wrap
  assert _state(c) == (-2 ** 31, -2 ** 31) and c.fresh(_GS(2 ** 31))


def test_a_stale_sync_under_capture_raises_and_touches_nothing(capturing):
  c = StepCounter('cpu', 'learning-rate')
  c.sync(_GS(12))
  capturing(True)
  with pytest.raises(RuntimeError) as e:
    c.sync(_GS(345))
  msg = str(e.value)
  assert 'learning-rate' in msg and 'counter (12)' in msg and 'global_step (345)' in msg
  assert msg.endswith('run one eager step after changing global_step')
  assert _state(c) == (12, 12)
  capturing(False)                                    # the eager step the message asks for repairs it
  c.sync(_GS(345))
  assert _state(c) == (345, 345)


def test_moved_wraps_and_is_undone():
  c = StepCounter('cpu', 'test')
  c.mirror = 2 ** 31 - 1
  c.moved(1)
  assert c.mirror == -2 ** 31 and c.fresh(_GS(2 ** 31))
  c.moved(-1)
  assert c.mirror == 2 ** 31 - 1
  assert int(c.tensor[0]) == 0                        # the mirror's moves never write the device


def test_summaries_pair_the_mirror_with_the_ledger():
  """TrainingSummaries needs a graph on the GPU; its ``fresh`` / ``moved`` read two host objects, so they run on a stub."""
  class Stub:
    fresh, moved = summaries.TrainingSummaries.fresh, summaries.TrainingSummaries.moved

    def __init__(self):
      self._ledger, self.counter = summaries.RingLedger(4), StepCounter('cpu', "summaries'")
  s = Stub()
  s.counter.mirror = 9
  assert s.fresh(_GS(9)) and not s.fresh(_GS(10))
  s.moved(1)                                          # a replay (or a launch of the hook) wrote step 9 ...
  assert s.counter.mirror == 10
  s.moved(1)                                          # ... and step 10
  s.moved(-1)                                         # a capture's host side is undone: step 10 was never written
  assert s.counter.mirror == 10
  assert s._ledger.take() == ([(9 % 4, 9)], 0)
  s.moved(1)
  s.moved(-1)
  assert s._ledger.take() == ([], 0) and s.counter.mirror == 10
  with pytest.raises(RuntimeError):
    s.moved(-1)                                       # nothing to undo: the ledger refuses, before the mirror moves
  assert s.counter.mirror == 10
  with pytest.raises(ValueError):
    s.moved(2)
  assert s.counter.mirror == 10
