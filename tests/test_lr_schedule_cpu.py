"""rigl_amd.schedules on the host: the twin every device result is compared with, against the records
tests/golden/make_golden_lr.py took from the reference's own lr_schedule (tests/golden/lr_schedule.npz)."""
import numpy as np
import pytest

from tests import lr_ref as R
from rigl_amd import schedules as S

F = np.float32


def _twin_bits(sched, steps):
  with np.errstate(all='ignore'):
    return np.array([R.bits(sched.value32(int(t))) for t in steps], dtype=np.uint32)


def test_golden_covers_what_it_should():
  meta, cases = R.golden()
  flags = [c[0] for c in cases]
  assert {f['arch'] for f in flags} == {'resnet', 'mobilenet_v1', 'vgg_16'}
  assert {f['multiplier'] for f in flags} >= {1.0, 0.5}
  assert {f['batch'] for f in flags} == {256, 4096}
  assert {f['sgdr'] for f in flags} == {False, True}
  for f, steps, _ in cases:
    assert {0, 1, 2 ** 24 + 1} <= set(steps.tolist()) and len(steps) >= 60, f


def test_arithmetic_schedules_match_the_reference_bit_for_bit():
  meta, cases = R.golden()
  n = 0
  for flags, steps, want in cases:
    if flags['sgdr']:
      continue
    got = _twin_bits(R.schedule_for(flags, meta), steps)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (flags, steps[bad][:5], got[bad][:5], want[bad][:5])
    n += 1
  assert n == len(cases) // 2


def test_sgdr_matches_the_reference_within_the_cosine_bound():
  """|lr - lr_ref| <= 2^-22 * lr0 * m_fac: one fp32 ulp of a cosine of magnitude <= 1 is 2^-24, then three more roundings of
  values <= 2; both sides round a double-precision cosine once."""
  meta, cases = R.golden()
  differing = total = 0
  for flags, steps, want in cases:
    if not flags['sgdr']:
      continue
    got = _twin_bits(R.schedule_for(flags, meta), steps)
    differing += int((got != want).sum())
    total += len(steps)
    for t, a, b in zip(steps, got.view(np.float32).astype(np.float64), want.view(np.float32).astype(np.float64)):
      lr0, m_fac = R.sgdr_cycle(flags, meta, int(t))
      assert abs(a - b) <= 2.0 ** -22 * lr0 * m_fac, (flags, int(t), a, b)
  print('SGDR: %d of %d recorded steps differ from the reference in any bit' % (differing, total))
  assert total > 0


def test_restatement_matches_and_every_mutant_is_rejected():
  """The records tell the comparison (<) and the warm-up's operation order apart: a restatement of the reference function
  reproduces them, and each mutation of it fails on at least one record."""
  meta, cases = R.golden()
  wrong = {m: 0 for m in (None,) + R.MUTATIONS}
  for flags, steps, want in cases:
    if flags['sgdr']:
      continue
    for m in wrong:
      got = np.array([R.bits(R.reference_chain(flags, meta, int(t), m)) for t in steps], dtype=np.uint32)
      wrong[m] += int((got != want).sum())
  assert wrong[None] == 0
  for m in R.MUTATIONS:
    assert wrong[m] > 0, 'the golden records do not reject the mutant %r' % m
  assert {'le_in_chain', 'warmup_divides_first'} <= set(R.MUTATIONS)


def test_resnet_chain_is_finite_at_step_0():
  s = S.imagenet_lr_schedule(0.1, 1024)
  assert s.segments[0]['kind'] == S.WARMUP and s.segments[0]['d'] == 0      # the warm-up divides by its start epoch 0 ...
  assert R.bits(s.value32(0)) == R.bits(F(0.1 * (1024 / 256.0)))            # ... and is never selected
  assert s(0) == float(F(0.4))


def test_piecewise_constant_follows_tfs_rule():
  s = S.piecewise_constant([10, 20], [1.0, 0.5, 0.25])
  # tf.train.piecewise_constant: x <= b keeps the old value
  assert [s(t) for t in (0, 9, 10, 11, 19, 20, 21, 10 ** 6)] == [1.0, 1.0, 1.0, 0.5, 0.5, 0.5, 0.25, 0.25]
  assert [g['start'] for g in s.segments[1:]] == [11, 21]
  e = S.piecewise_constant([], [0.3])
  assert R.bits(e.value32(0)) == R.bits(F(0.3)) == R.bits(e.value32(R.INT32_MAX)) and len(e.segments) == 1
  d = S.piecewise_constant([5, 5], [1.0, 2.0, 3.0])        # an empty middle interval: TF's value above the boundary wins
  assert [d(t) for t in (5, 6)] == [1.0, 3.0]
  assert S.piecewise_constant([0], [1.0, 2.0])(0) == 1.0


def test_cifar_and_mnist_builders_are_the_reference_lines():
  c = S.cifar_lr_schedule()
  vals = [0.1 / (5. ** i) for i in range(4)]                                # resnet_train_eval.py:199
  for t, v in [(0, vals[0]), (30000, vals[0]), (30001, vals[1]), (60000, vals[1]), (60001, vals[2]), (90000, vals[2]),
               (90001, vals[3]), (10 ** 7, vals[3])]:
    assert R.bits(c.value32(t)) == R.bits(F(v)), t
  h = S.cifar_lr_schedule(0.5)
  assert [g['start'] for g in h.segments[1:]] == [15001, 30001, 45001]
  m = S.mnist_lr_schedule(0.2, 550)                                         # mnist_train_eval.py:249-256
  assert [g['start'] for g in m.segments[1:]] == [60 * 550 + 1, 70 * 550 + 1, 80 * 550 + 1]
  assert [R.bits(g['c']) for g in m.segments] == [R.bits(F(0.2 / (3. ** i))) for i in range(4)]
  p = S.mnist_lr_schedule(0.2, 550, use_model_pruning=True, lr_drop_epoch=75)
  assert [g['start'] for g in p.segments[1:]] == [75 * 550 + 1, 95 * 550 + 1]
  assert [R.bits(g['c']) for g in p.segments] == [R.bits(F(0.2 / (3. ** i))) for i in range(3)]


def test_cosine_decay_is_the_one_cycle_case():
  s = S.cosine_decay(0.5, 100)
  assert s(0) == 0.5
  for t in (1, 37, 99):
    want = F(0.5) * (F(0.5) * (F(1.0) + F(np.cos(np.float64(F(R.PI) * (F(t) / F(100)))))))
    assert R.bits(s.value32(t)) == R.bits(want), t
  assert s(100) == s(10 ** 6) == float(F(0.5) * (F(0.5) * (F(1.0) + F(np.cos(np.float64(F(R.PI)))))))
  r = S.cosine_decay_restarts(0.5, 100, t_mul=1.0, m_mul=1.0, total_steps=100)
  assert all(R.bits(r.value32(t)) == R.bits(s.value32(t)) for t in range(100))


def test_cosine_decay_restarts_cycles():
  s = S.cosine_decay_restarts(1.0, 10, t_mul=2.0, m_mul=0.5, total_steps=70)
  assert [g['start'] for g in s.segments[1:]] == [10, 30]                    # cycles of 10, 20 and 40 steps cover 70
  assert [s(t) for t in (0, 10, 30)] == [1.0, 0.5, 0.25]                      # each restart begins at lr0 * m_mul^i
  assert s(9) < 0.03 and s(29) < 0.01


def test_builders_refuse_what_the_table_cannot_hold():
  with pytest.raises(ValueError, match='segments'):
    S.piecewise_constant(list(range(1, 33)), [0.1] * 33)                     # 33 segments
  S.piecewise_constant(list(range(1, 32)), [0.1] * 32)                       # 32 fit
  with pytest.raises(ValueError, match='sorted'):
    S.piecewise_constant([20, 10], [1.0, 0.5, 0.25])
  with pytest.raises(ValueError, match='one more'):
    S.piecewise_constant([10], [1.0])
  with pytest.raises(ValueError, match='int32'):
    S.piecewise_constant([R.INT32_MAX], [1.0, 0.5])                          # b + 1 does not fit the counter
  with pytest.raises(ValueError, match='total_steps'):
    S.cosine_decay_restarts(0.1, 10)
  with pytest.raises(ValueError, match='cycles'):
    S.cosine_decay_restarts(0.1, 10, t_mul=1.0, total_steps=10 * 33)
  with pytest.raises(ValueError, match='train_steps'):
    S.imagenet_lr_schedule(0.1, 256, use_sgdr=True)
  with pytest.raises(ValueError, match='Unknown architecture'):
    S.imagenet_lr_schedule(0.1, 256, model_architecture='alexnet')


def test_descriptor_holds_the_table():
  s = S.imagenet_lr_schedule(0.1, 4096, model_architecture='mobilenet_v1')
  d = s.descriptor()
  assert d is s.descriptor()
  assert (d.n_seg, d.domain) == (6, S.EPOCH) and R.bits(d.steps_per_epoch) == R.bits(F(1281167 / 4096))
  assert [d.seg[i].kind for i in range(6)] == [S.WARMUP] + [S.CONST] * 5
  assert [d.seg[i].start for i in range(1, 6)] == [8.0, 40.0, 75.0, 95.0, 120.0] and d.seg[0].start == -np.inf
  assert R.bits(d.seg[0].c) == R.bits(F(1.6)) and d.seg[0].d == 8.0
  p = S.piecewise_constant([10], [1.0, 0.5]).descriptor()
  assert (p.n_seg, p.domain, p.seg[0].start_step, p.seg[1].start_step) == (2, S.STEP, -2 ** 31, 11)


def test_host_faces_and_the_alias():
  from rigl.imagenet_resnet import imagenet_train_eval
  assert imagenet_train_eval.imagenet_lr_schedule is S.imagenet_lr_schedule
  s = S.cifar_lr_schedule()
  h = s.host_only()
  assert callable(h) and not isinstance(h, S.Schedule) and h(30001) == s(30001)
  assert s.value32(2 ** 31) == s.value32(-2 ** 31)                           # the int32 counter wraps


def test_optimizer_takes_the_host_path_without_a_gpu_graph():
  """A Schedule on a CPU graph (and host_only() anywhere) is an ordinary callable learning rate."""
  from rigl_amd import step_state, train
  s = S.piecewise_constant([1], [0.5, 0.25])

  class GS:
    value = 2
  assert train._lr_value(s, GS) == 0.25 and train._lr_value(s.host_only(), GS) == 0.25
  assert step_state.int32(2 ** 31) == -2 ** 31 and step_state.int32(-1) == -1
