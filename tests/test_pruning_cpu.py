"""Gradual magnitude pruning, host side: contrib's hyperparameters, the
sparsity schedule, the update gate, the per-layer k, the weight_sparsity_map
rules, and the NumPy restatement (tests/prune_ref.py) against the golden cases
(tests/golden/prune_cases.npz, written by make_golden_prune.py)."""
import os

import numpy as np
import pytest

import prune_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'prune_cases.npz')
F32 = np.float32
CASES = ('random', 'ties', 'zeros_denormals', 'k_extremes', 'decay05', 'decay0_old')


def _graph(layers=(('layer1', (784, 300)), ('layer2', (300, 100)), ('layer3', (100, 10)))):
  from rigl_amd import variables as V
  g = V.Graph('cpu')
  for scope, shape in layers:
    g.add_masked_layer(scope, shape, True)
  g.finalize()
  return g


def test_hparam_defaults():
  from rigl_amd import pruning
  h = pruning.get_pruning_hparams()
  assert h.values() == dict(
      name='model_pruning', begin_pruning_step=0, end_pruning_step=-1, weight_sparsity_map=[''],
      threshold_decay=0.0, pruning_frequency=10, nbins=256, block_height=1, block_width=1,
      block_pooling_function='AVG', initial_sparsity=0.0, target_sparsity=0.5, sparsity_function_begin_step=0,
      sparsity_function_end_step=100, sparsity_function_exponent=3, use_tpu=False, prune_option='weight')


def test_hparam_parse_as_the_drivers_write_it():
  from rigl_amd import pruning
  # mnist_train_eval.py:320-337
  h = pruning.get_pruning_hparams().parse(
      'begin_pruning_step=2000,sparsity_function_begin_step=2000,end_pruning_step=30000,'
      'sparsity_function_end_step=30000,target_sparsity=0.98,pruning_frequency=500,threshold_decay=0')
  h.set_hparam('weight_sparsity_map', ['layer2:0.98', 'layer3:0.0'])
  assert (h.begin_pruning_step, h.end_pruning_step, h.pruning_frequency) == (2000, 30000, 500)
  assert isinstance(h.threshold_decay, float) and h.threshold_decay == 0.0
  assert h.target_sparsity == 0.98 and h.weight_sparsity_map == ['layer2:0.98', 'layer3:0.0']
  # resnet_train_eval.py:249-275 passes use_tpu=False
  h = pruning.get_pruning_hparams().parse('threshold_decay=0,use_tpu=False,weight_sparsity_map=[a:0.5,b:0.25]')
  assert h.use_tpu is False and h.weight_sparsity_map == ['a:0.5', 'b:0.25']
  assert pruning.get_pruning_hparams().parse('use_tpu=true').use_tpu is True


def test_hparam_unknown_names_and_bad_values_raise():
  from rigl_amd import pruning
  with pytest.raises(ValueError):
    pruning.get_pruning_hparams().parse('no_such_param=1')
  with pytest.raises(ValueError):
    pruning.get_pruning_hparams().set_hparam('no_such_param', 1)
  with pytest.raises(ValueError):
    pruning.get_pruning_hparams().parse('pruning_frequency=2.5')
  with pytest.raises(ValueError):
    pruning.get_pruning_hparams().parse('use_tpu=maybe')


@pytest.mark.parametrize('step,expect', [(0, 0.0), (2000, 0.0), (30000, 0.98), (40000, 0.98)])
def test_schedule_before_begin_at_end_and_after(step, expect):
  from rigl_amd import pruning
  h = pruning.get_pruning_hparams().parse('sparsity_function_begin_step=2000,sparsity_function_end_step=30000,'
                                          'target_sparsity=0.98')
  assert pruning.schedule_sparsity(h, step) == F32(expect)


def test_schedule_middle_is_the_cubic_in_fp32():
  from rigl_amd import pruning
  h = pruning.get_pruning_hparams().parse('sparsity_function_begin_step=4,sparsity_function_end_step=40,'
                                          'target_sparsity=0.9')
  for t in range(0, 60):
    s = pruning.schedule_sparsity(h, t)
    assert s.dtype == np.float32
    assert s.view(np.uint32) == R.sparsity(t, 0.0, 0.9, 4, 40, 3).view(np.uint32)
  p = F32(F32(22 - 4) / F32(36))
  assert pruning.schedule_sparsity(h, 22) == F32(F32(F32(-0.9) * F32(np.power(F32(1) - p, F32(3)))) + F32(0.9))
  assert F32(0) < pruning.schedule_sparsity(h, 5) < pruning.schedule_sparsity(h, 39) < F32(0.9)


def test_gate_range_frequency_and_negative_end():
  from rigl_amd import pruning
  g = _graph()
  gs = g.get_or_create_global_step()
  h = pruning.get_pruning_hparams().parse('begin_pruning_step=4,end_pruning_step=40,pruning_frequency=4')
  p = pruning.Pruning(h, global_step=gs, graph=g)
  fired = [t for t in range(0, 60) if p.should_update(t)]
  assert fired == list(range(4, 41))                       # last_mask_update_step still 0: frequency satisfied
  p._state.last_mask_update_step.fill_(8)                  # pylint: disable=protected-access
  assert not p.should_update(11) and p.should_update(12) and not p.should_update(41)
  h2 = pruning.get_pruning_hparams().parse('begin_pruning_step=4,end_pruning_step=-1,pruning_frequency=4')
  p2 = pruning.Pruning(h2, global_step=gs, graph=g)
  assert p2.should_update(10 ** 7) and not p2.should_update(3)
  for t in range(0, 100):
    for last in (0, 5, 37):
      p._state.last_mask_update_step.fill_(last)          # pylint: disable=protected-access
      assert p.should_update(t) == R.gate(t, last, 4, 40, 4)


def test_k_rounds_half_to_even():
  from rigl_amd import pruning
  assert F32(2) * (F32(1) - F32(0.25)) == F32(1.5)           # exact fp32 halves
  assert pruning.num_kept(2, F32(0.25)) == 2
  assert pruning.num_kept(6, F32(0.25)) == 4
  assert pruning.num_kept(10, F32(0.25)) == 8               # 7.5 -> 8
  assert pruning.num_kept(6, F32(0.25)) == R.k_of(6, 0.25) and pruning.num_kept(2, F32(0.25)) == R.k_of(2, 0.25)
  with pytest.raises(ValueError):
    pruning.num_kept(100, F32(1.0))                         # k == 0: contrib's gather(values, -1)
  with pytest.raises(ValueError):
    pruning.num_kept(1, F32(0.6))                           # 0.4 rounds to 0


def test_weight_sparsity_map_substrings_and_multiple_matches():
  from rigl_amd import pruning
  g = _graph()
  gs = g.get_or_create_global_step()
  h = pruning.get_pruning_hparams().parse('target_sparsity=0.9,sparsity_function_begin_step=0,'
                                          'sparsity_function_end_step=10')
  h.set_hparam('weight_sparsity_map', ['layer2:0.45', 'layer3:0'])
  p = pruning.Pruning(h, global_step=gs, graph=g)
  gs.assign(10)
  ks = [k for _, k in p.layer_ks()]
  s = F32(0.9)
  assert ks == [R.k_of(784 * 300, s), R.k_of(300 * 100, R.layer_sparsity('layer2/weights', s, {'layer2': 0.45}, 0.9)),
                100 * 10]
  assert ks[1] == 300 * 100 - int(np.rint(F32(F32(30000) * F32(0.45))))
  h.set_hparam('weight_sparsity_map', ['layer:0.5', 'layer2:0.45'])
  with pytest.raises(ValueError, match='Multiple matches'):
    pruning.Pruning(h, global_step=gs, graph=g).layer_ks()
  h.set_hparam('weight_sparsity_map', ['layer1:0.99999'])
  with pytest.raises(ValueError):                           # s_l = 0.99999 on 4 weights: k == 0
    pruning.Pruning(h, global_step=gs, graph=_graph((('layer1', (2, 2)),))).layer_ks()


@pytest.mark.parametrize('opt', ['block_height=2', 'block_width=4', 'use_tpu=True', 'prune_option=first_order_gradient'])
def test_options_outside_the_restatement_raise(opt):
  from rigl_amd import pruning
  with pytest.raises(NotImplementedError):
    pruning.Pruning(pruning.get_pruning_hparams().parse(opt), graph=_graph())


def test_threshold_state_only_with_a_pruning_object():
  from rigl_amd import pruning, tf_checkpoint
  g = _graph()
  before = sorted(tf_checkpoint.variable_map(g))
  assert pruning.get_thresholds(g) == [] and not hasattr(g, 'pruning_state')
  pruning.Pruning(graph=g)
  after = sorted(tf_checkpoint.variable_map(g))
  assert sorted(set(after) - set(before)) == ['layer1/threshold', 'layer2/threshold', 'layer3/threshold',
                                              'model_pruning/last_mask_update_step']
  assert [float(t) for t in pruning.get_thresholds(g)] == [0.0, 0.0, 0.0]
  assert [float(s) for s in pruning.get_weight_sparsity(g)] == [0.0, 0.0, 0.0]


@pytest.mark.parametrize('case', CASES)
def test_restatement_reproduces_the_golden_cases(case):
  t = np.load(GOLDEN)
  decay = float(t[case + '__decay'])
  for i in range(int(t[case + '__n_layers'])):
    p = '%s__L%d_' % (case, i)
    w, k = t[p + 'w'], int(t[p + 'k'])
    thr, mask = R.mask_update(w, k, t[p + 'thr_old'], decay)
    assert thr.view(np.uint32) == t[p + 'thr'].view(np.uint32)
    np.testing.assert_array_equal(R.pack_bits(mask), t[p + 'mask'])
    assert int(mask.sum()) == int(t[p + 'ones'])
    if decay == 0.0:
      assert int(mask.sum()) >= k                          # every tie of the k-th value is admitted


def test_golden_ties_and_denormals_are_exercised():
  t = np.load(GOLDEN)
  assert any(int(t['ties__L%d_ones' % i]) > int(t['ties__L%d_k' % i]) for i in range(4))
  thr = [float(t['zeros_denormals__L%d_thr' % i]) for i in range(9)]
  assert any(0 < x < 1.1754944e-38 for x in thr) and 0.0 in thr


@pytest.mark.parametrize('tag', ['mnist', 'defaults'])
def test_host_schedule_matches_the_golden_trace(tag):
  from rigl_amd import pruning
  t = np.load(GOLDEN)
  p = 'sched_%s__' % tag
  if tag == 'mnist':
    h = pruning.get_pruning_hparams().parse(
        'begin_pruning_step=4,sparsity_function_begin_step=4,end_pruning_step=40,sparsity_function_end_step=40,'
        'target_sparsity=0.9,pruning_frequency=4,threshold_decay=0')
    h.set_hparam('weight_sparsity_map', ['layer2:0.45', 'layer3:0.0'])
    g = _graph()
  else:
    h = pruning.get_pruning_hparams()
    g = _graph((('conv1', (3, 3, 3, 16)), ('fc', (64, 10))))
  gs = g.get_or_create_global_step()
  pr = pruning.Pruning(h, global_step=gs, graph=g)
  for i, step in enumerate(t[p + 'steps']):
    gs.assign(int(step))
    assert pr.sparsity.view(np.uint32) == t[p + 's'][i].view(np.uint32)
    assert [k for _, k in pr.layer_ks()] == list(t[p + 'k'][i])
    fire = pr.should_update()
    assert fire == bool(t[p + 'gate'][i])
    if fire:
      pr._state.last_mask_update_step.fill_(int(step))     # pylint: disable=protected-access  (what the update sets)
