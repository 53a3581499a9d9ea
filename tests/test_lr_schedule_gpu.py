"""rigl_lr_schedule_step on the device against the host twin (rigl_amd.schedules): the arithmetic-only schedules bit for
bit, the cosine within its rounding bound, the counter's advance, a thousand launches in a row, and every refusal."""
import ctypes as C
import math

import numpy as np
import pytest

torch = pytest.importorskip('torch')

from tests import lr_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
INT32_MAX = R.INT32_MAX


def _device_values(sched, steps):
  """One launch per step with the counter uploaded to it -> (lr bits uint32 [k], counter afterwards int64 [k])."""
  from rigl_amd import ops
  step = torch.zeros(1, dtype=torch.int32, device=DEV)
  lr = torch.zeros(1, dtype=torch.float32, device=DEV)
  got = torch.empty(len(steps), dtype=torch.float32, device=DEV)
  after = torch.empty(len(steps), dtype=torch.int32, device=DEV)
  d = sched.descriptor()
  for i, s in enumerate(steps):
    step.fill_(int(s))
    lr.fill_(float('nan'))
    ops.lr_schedule_step(d, step, lr)
    got[i:i + 1].copy_(lr)
    after[i:i + 1].copy_(step)
  torch.cuda.synchronize()
  return got.cpu().numpy().view(np.uint32), after.cpu().numpy().astype(np.int64)


def _host_bits(sched, steps):
  with np.errstate(all='ignore'):
    return np.array([R.bits(sched.value32(int(s))) for s in steps], dtype=np.uint32)


def _boundary_steps(sched):
  """The first step at or above every start of the table (the step where the active segment changes)."""
  from rigl_amd import schedules as S
  out = []
  for i in range(1, len(sched.segments)):
    st = sched.segments[i]['start']
    if sched.domain == S.STEP:
      out.append(int(st))
      continue
    s = max(int(math.ceil(float(st) * float(sched.steps_per_epoch))), 0)
    while s > 0 and not sched.active_segment(s - 1)[1] < st:
      s -= 1
    while sched.active_segment(s)[1] < st:
      s += 1
    out.append(s)
  return out


def _steps_for(sched):
  steps = {0, 2 ** 24 + 1, INT32_MAX}
  for b in _boundary_steps(sched):
    steps.update(s for s in (b - 1, b, b + 1) if 0 <= s <= INT32_MAX)
  return sorted(steps)


def _arithmetic_schedules():
  from rigl_amd import schedules as S
  return {
      'imagenet_resnet': S.imagenet_lr_schedule(0.1, 1024),
      'imagenet_resnet_half': S.imagenet_lr_schedule(0.1, 256, training_steps_multiplier=0.5),
      'imagenet_mobilenet': S.imagenet_lr_schedule(0.1, 4096, model_architecture='mobilenet_v1'),
      'imagenet_mobilenet_0.3': S.imagenet_lr_schedule(0.1, 256, model_architecture='mobilenet_v1',
                                                       training_steps_multiplier=0.3),
      'cifar': S.cifar_lr_schedule(),
      'one_segment': S.piecewise_constant([], [0.3]),
      '32_segments': S.piecewise_constant([7 * i for i in range(1, 32)], [0.5 / (i + 1) for i in range(32)]),
  }


@pytest.mark.parametrize('name', ['imagenet_resnet', 'imagenet_resnet_half', 'imagenet_mobilenet', 'imagenet_mobilenet_0.3',
                                  'cifar', 'one_segment', '32_segments'])
def test_arithmetic_schedules_are_bit_exact(name):
  sched = _arithmetic_schedules()[name]
  steps = _steps_for(sched)
  if name == 'imagenet_mobilenet_0.3':
    steps = sorted(set(steps) | set(range(1, 12000, 397)))       # inside the warm-up, whose divisor 2.4 is no power of two
  got, after = _device_values(sched, steps)
  want = _host_bits(sched, steps)
  bad = np.nonzero(got != want)[0]
  assert bad.size == 0, (name, [steps[i] for i in bad[:5]], got[bad][:5], want[bad][:5])
  assert after.tolist() == [((s + 1 + 2 ** 31) % 2 ** 32) - 2 ** 31 for s in steps]     # INT32_MAX wraps to INT32_MIN
  if name == 'imagenet_resnet':
    lr0 = got.view(np.float32)[steps.index(0)]
    assert np.isfinite(lr0) and R.bits(lr0) == R.bits(np.float32(0.1 * (1024 / 256.0)))  # the warm-up's divisor is 0


def _cosine_schedules():
  from rigl_amd import schedules as S
  return {
      'steps': S.cosine_decay_restarts(0.1, 100, t_mul=2.0, m_mul=0.5, total_steps=1600),
      'steps_t1': S.cosine_decay_restarts(0.3, 64, t_mul=1.0, m_mul=0.9, total_steps=64 * 5),
      'one_cycle': S.cosine_decay(0.2, 1000),
      'imagenet_sgdr': S.imagenet_lr_schedule(0.1, 1024, use_sgdr=True, train_steps=112590),
  }


@pytest.mark.parametrize('name', ['steps', 'steps_t1', 'one_cycle', 'imagenet_sgdr'])
def test_cosine_is_within_its_rounding_bound(name):
  """|lr_dev - lr_host| <= 2^-22 * lr0 * m_fac per step: one fp32 ulp of a cosine of magnitude <= 1 is 2^-24, then three
  more roundings of values <= 2; both sides round a double-precision cosine once."""
  from rigl_amd import schedules as S
  sched = _cosine_schedules()[name]
  bounds = [0] + _boundary_steps(sched)
  steps = set()
  for k, b in enumerate(bounds[:5]):                             # the first and the last step of each of the first four cycles
    steps.add(b)
    if k > 0:
      steps.add(b - 1)
  steps.update(range(3, bounds[min(4, len(bounds) - 1)] + 50, 37))
  steps = sorted(steps)
  got, after = _device_values(sched, steps)
  want = _host_bits(sched, steps)
  print('%s: %d of %d steps differ from the host twin in any bit' % (name, int((got != want).sum()), len(steps)))
  assert after.tolist() == [s + 1 for s in steps]
  for s, a, b in zip(steps, got.view(np.float32).astype(np.float64), want.view(np.float32).astype(np.float64)):
    g = sched.segments[sched.active_segment(s)[0]]
    scale = float(g['c']) * (float(g['m_fac']) if g['kind'] == S.COSINE else 1.0)
    assert abs(a - b) <= 2.0 ** -22 * scale, (name, s, a, b)


def test_a_thousand_launches_in_a_row_stay_in_step():
  """No upload in between: launch k evaluates step k and leaves k + 1 -- through the warm-up (steps 0..599) and past it."""
  from rigl_amd import ops, schedules as S
  sched = S.imagenet_lr_schedule(0.1, 256, num_train_images=256 * 75, model_architecture='mobilenet_v1')
  step = torch.zeros(1, dtype=torch.int32, device=DEV)
  lr = torch.zeros(1, dtype=torch.float32, device=DEV)
  got = torch.empty(1000, dtype=torch.float32, device=DEV)
  d = sched.descriptor()
  for i in range(1000):
    ops.lr_schedule_step(d, step, lr)
    got[i:i + 1].copy_(lr)
  torch.cuda.synchronize()
  assert int(step.item()) == 1000
  want = _host_bits(sched, range(1000))
  assert sched.active_segment(599)[0] == 0 and sched.active_segment(600)[0] == 1
  np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want)


def _desc(n_seg=2, domain=0, spe=0.0, kinds=(0, 0), starts=(0, 5), lens=None):
  from rigl_amd import _lib
  d = _lib.LrSchedule()
  d.n_seg, d.domain, d.steps_per_epoch = n_seg, domain, spe
  for i, k in enumerate(kinds):
    g = d.seg[i]
    g.kind, g.c, g.d, g.sum_r, g.len, g.m_fac = k, 0.1, 1.0, 0.0, (lens[i] if lens else 1.0), 1.0
    g.start_step, g.start = (int(starts[i]) if math.isfinite(starts[i]) else 0), float(starts[i])
  return d


def test_every_bad_argument_is_refused_before_a_launch():
  from rigl_amd import _lib, ops
  lib = _lib.load()
  step = torch.full((2,), 1234, dtype=torch.int32, device=DEV)
  lr = torch.full((2,), -7.0, dtype=torch.float32, device=DEV)
  sp, lp = step.data_ptr(), lr.data_ptr()
  ok = _desc()
  nan, inf = float('nan'), float('inf')
  bad = {
      'NULL sched': (None, sp, lp),
      'NULL step': (C.byref(ok), None, lp),
      'NULL lr_out': (C.byref(ok), sp, None),
      'misaligned step': (C.byref(ok), sp + 2, lp),
      'misaligned lr_out': (C.byref(ok), sp, lp + 1),
      'n_seg 0': (C.byref(_desc(n_seg=0)), sp, lp),
      'n_seg 33': (C.byref(_desc(n_seg=33)), sp, lp),
      'n_seg -1': (C.byref(_desc(n_seg=-1)), sp, lp),
      'descending step starts': (C.byref(_desc(starts=(5, 4))), sp, lp),
      'descending epoch starts': (C.byref(_desc(domain=1, spe=10.0, starts=(2.5, 2.25))), sp, lp),
      'NaN epoch start': (C.byref(_desc(domain=1, spe=10.0, starts=(0.0, nan))), sp, lp),
      'steps_per_epoch 0': (C.byref(_desc(domain=1, spe=0.0)), sp, lp),
      'steps_per_epoch < 0': (C.byref(_desc(domain=1, spe=-3.0)), sp, lp),
      'steps_per_epoch inf': (C.byref(_desc(domain=1, spe=inf)), sp, lp),
      'steps_per_epoch NaN': (C.byref(_desc(domain=1, spe=nan)), sp, lp),
      'unknown kind': (C.byref(_desc(kinds=(0, 3))), sp, lp),
      'negative kind': (C.byref(_desc(kinds=(-1, 0))), sp, lp),
      'unknown domain': (C.byref(_desc(domain=2, spe=1.0)), sp, lp),
      'cosine len 0': (C.byref(_desc(kinds=(2, 0), lens=(0.0, 1.0))), sp, lp),
      'cosine len < 0': (C.byref(_desc(kinds=(0, 2), lens=(1.0, -1.0))), sp, lp),
      'cosine len NaN': (C.byref(_desc(kinds=(2, 0), lens=(nan, 1.0))), sp, lp),
  }
  for what, (d, s, l) in bad.items():
    assert lib.rigl_lr_schedule_step(d, s, l, None) == _lib.RIGL_EINVAL, what
    assert b'rigl_lr_schedule_step' in lib.rigl_last_error(), what
  torch.cuda.synchronize()
  assert step.cpu().tolist() == [1234, 1234] and lr.cpu().tolist() == [-7.0, -7.0]
  # equal starts ascend; the step domain ignores steps_per_epoch; a CONST segment ignores len
  for d in (_desc(starts=(5, 5)), _desc(spe=nan), _desc(lens=(0.0, -1.0))):
    assert lib.rigl_lr_schedule_step(C.byref(d), sp, lp, None) == _lib.RIGL_OK
  torch.cuda.synchronize()
  assert step.cpu().tolist() == [1237, 1234] and lr.cpu().tolist()[1] == -7.0
  # the tensor-level wrapper
  with pytest.raises(TypeError):
    ops.lr_schedule_step(ok, step[:1].float(), lr[:1])
  with pytest.raises(TypeError):
    ops.lr_schedule_step('schedule', step[:1], lr[:1])
  with pytest.raises(ValueError):
    ops.lr_schedule_step(ok, step, lr[:1])
  with pytest.raises(Exception, match='GPU'):
    ops.lr_schedule_step(ok, step[:1].cpu(), lr[:1])
