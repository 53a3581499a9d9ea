"""rigl_magnitude_prune_batched and rigl_amd.pruning on the GPU: the kernel
against the golden cases bit for bit (thresholds as bits, bitmaps, counts,
weights untouched), one call over ResNet-50's 54 masked tensors against NumPy,
an MNIST MLP prune run checked at every update against tests/prune_ref.py, eager
vs GraphedStep on WRN-22 with pruning between steps, and a checkpoint round trip
of the pruning state."""
import os

import numpy as np
import pytest

import prune_ref as R

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'prune_cases.npz')
CASES = ('random', 'ties', 'zeros_denormals', 'k_extremes', 'decay05', 'decay0_old')


def _words(bits_t, n):
  return bits_t.cpu().numpy().view(np.uint32)[:(n + 31) // 32]


@pytest.mark.parametrize('case', CASES)
def test_kernel_matches_the_golden_cases_bit_for_bit(case):
  from rigl_amd import ops
  t = np.load(GOLDEN)
  m = int(t[case + '__n_layers'])
  items, ws, ref = [], [], []
  for i in range(m):
    p = '%s__L%d_' % (case, i)
    w = torch.from_numpy(t[p + 'w'].copy()).to(DEV)
    bits = torch.from_numpy(t[p + 'mask_old'].view(np.int32).copy()).to(DEV)
    thr = torch.from_numpy(np.array([t[p + 'thr_old']], np.float32)).to(DEV)
    items.append((w, bits, thr, int(t[p + 'k'])))
    ws.append(w.clone())
    ref.append(p)
  counts = torch.full((m, 4), -1, dtype=torch.int32, device=DEV)
  ops.magnitude_prune_batched(items, float(t[case + '__decay']), counts)
  torch.cuda.synchronize()
  c = counts.cpu().numpy()
  for i, (w, bits, thr, k) in enumerate(items):
    p = ref[i]
    n = w.numel()
    assert thr.cpu().numpy().view(np.uint32)[0] == t[p + 'thr'].view(np.uint32), (p, 'threshold bits')
    np.testing.assert_array_equal(_words(bits, n), t[p + 'mask'], err_msg=p + ' bitmap')
    assert list(c[i]) == [n, k, int(t[p + 'ones']), int(t[p + 'ones_old'])], p
    assert torch.equal(w.view(torch.int32), ws[i].view(torch.int32)), p + ' weights changed'


def test_one_call_over_every_resnet50_masked_tensor():
  from rigl_amd import ops
  from tests.golden import layer_shapes
  shapes = list(layer_shapes.resnet50().values())
  assert len(shapes) == 54
  gen = torch.Generator(device=DEV).manual_seed(7)
  items, np_w = [], []
  for i, sh in enumerate(shapes):
    n = int(np.prod(sh))
    w = torch.randn(n, device=DEV, generator=gen) * 0.05
    if i % 3 == 0:
      w = (w * 64).round() / 64                             # heavy ties on a third of the layers
    bits = torch.zeros((n + 31) // 32, dtype=torch.int32, device=DEV)
    thr = torch.full((1,), 0.01 * (i % 4), dtype=torch.float32, device=DEV)
    s = (0.5, 0.8, 0.9, 0.95)[i % 4]
    items.append((w, bits, thr, R.k_of(n, s)))
    np_w.append((w.cpu().numpy(), float(thr.item())))
  assert max(it[0].numel() for it in items) == 3 * 3 * 512 * 512      # the 2.36 M-weight layer
  counts = torch.empty((len(items), 4), dtype=torch.int32, device=DEV)
  ops.magnitude_prune_batched(items, 0.5, counts)
  torch.cuda.synchronize()
  c = counts.cpu().numpy()
  for i, (w, bits, thr, k) in enumerate(items):
    t_ref, m_ref = R.mask_update(np_w[i][0], k, np_w[i][1], 0.5)
    assert thr.cpu().numpy().view(np.uint32)[0] == np.float32(t_ref).view(np.uint32), i
    np.testing.assert_array_equal(_words(bits, w.numel()), R.pack_bits(m_ref), err_msg='layer %d' % i)
    assert c[i, 2] == int(m_ref.sum()) and c[i, 0] == w.numel() and c[i, 1] == k


def _mnist_pruning(g, gs):
  from rigl_amd import pruning
  h = pruning.get_pruning_hparams().parse(
      'begin_pruning_step=4,sparsity_function_begin_step=4,end_pruning_step=40,sparsity_function_end_step=40,'
      'target_sparsity=0.9,pruning_frequency=4,threshold_decay=0')
  h.set_hparam('weight_sparsity_map', ['layer2:0.45', 'layer3:0.0'])     # mnist_train_eval.py:279-282, 320-337
  return pruning.Pruning(h, global_step=gs, graph=g)


def test_mnist_mlp_prune_run_follows_the_restatement():
  from rigl_amd import pruning, train, variables as V
  from rigl_amd.workloads import mnist_mlp
  g = V.reset_default_graph(DEV)
  model = mnist_mlp.MnistMLP(g)
  gs = g.get_or_create_global_step()
  opt = train.MomentumOptimizer(0.05, 0.9, use_nesterov=True, graph=g)
  p = _mnist_pruning(g, gs)
  x, y = mnist_mlp.synthetic_batch(64, DEV)
  layers = g.masked_layers()
  smap = {'layer2': 0.45, 'layer3': 0.0}
  thr = [np.float32(0)] * 3
  updates = []
  for _ in range(44):
    opt.minimize(model.loss(x, y), gs)
    t = int(gs.value)
    if not p.should_update():
      assert not p.conditional_mask_update_op()
      continue
    w_before = [l.weights.numpy().copy() for l in layers]
    assert p.conditional_mask_update_op()
    s = R.sparsity(t, 0.0, 0.9, 4, 40, 3)
    got_thr = [float(v) for v in pruning.get_thresholds(g)]
    for i, l in enumerate(layers):
      k = R.k_of(w_before[i].size, R.layer_sparsity(l.scope + '/weights', s, smap, 0.9))
      thr[i], m = R.mask_update(w_before[i], k, thr[i], 0.0)
      assert np.float32(got_thr[i]).view(np.uint32) == thr[i].view(np.uint32), (t, l.scope)
      np.testing.assert_array_equal(l.mask.numpy(), m.astype(np.float32), err_msg='%d %s' % (t, l.scope))
      np.testing.assert_array_equal(l.weights.numpy(), w_before[i])               # the update touches no weight
    updates.append((t, [int(l.mask.sum()) for l in layers],
                    [R.k_of(w_before[i].size, R.layer_sparsity(l.scope + '/weights', s, smap, 0.9))
                     for i, l in enumerate(layers)]))
  assert [u[0] for u in updates] == list(range(4, 41, 4))
  assert int(p._state.last_mask_update_step) == 40                          # pylint: disable=protected-access
  t_last, ones, ks = updates[-1]
  assert t_last == 40 and p.sparsity == np.float32(0.9)                     # the last update reaches the target
  assert ks == [R.k_of(235200, np.float32(0.9)), 16500, 1000]
  assert ones[0] >= ks[0] and ones[1] >= ks[1] and ones[2] == 1000          # ties only ever add; layer3 stays dense
  assert layers[2].mask.numpy().all()
  sp = pruning.get_weight_sparsity(g)
  assert abs(float(sp[0]) - 0.9) < 1e-3 and abs(float(sp[1]) - 0.45) < 1e-3 and float(sp[2]) == 0.0


def _wrn_run(graphed, steps):
  from rigl_amd import pruning, train, variables as V
  from rigl_amd.workloads import wide_resnet
  g = V.reset_default_graph(DEV)
  model = wide_resnet.WideResNet(g, depth=22, width=1)
  gs = g.get_or_create_global_step()
  inner = train.MomentumOptimizer(0.05, 0.9, use_nesterov=True, graph=g)
  h = pruning.get_pruning_hparams().parse('begin_pruning_step=3,sparsity_function_begin_step=3,end_pruning_step=30,'
                                          'sparsity_function_end_step=30,target_sparsity=0.8,pruning_frequency=3,'
                                          'threshold_decay=0.5')
  pr = pruning.Pruning(h, global_step=gs, graph=g)
  x, y = wide_resnet.synthetic_batch(32, DEV)
  loss_fn = lambda: model.loss(x, y)
  st = train.GraphedStep(loss_fn, inner, gs, warmup=1) if graphed else None
  fired = 0
  for _ in range(steps):
    if st is not None:
      st()
    else:
      inner.minimize(loss_fn(), gs)
    fired += int(pr.conditional_mask_update_op())       # under control_dependencies([train_op]): after the step
  torch.cuda.synchronize()
  out = dict(W=g.W.cpu().numpy().copy(), B=g.BITS.cpu().numpy().copy(),
             T=g.pruning_state.thresholds.cpu().numpy().copy(), gs=int(gs.value), fired=fired)
  if st is not None:
    out['replays'] = st.replays
  return out


def test_wrn22_pruning_between_graph_replays_matches_eager():
  steps = 20
  a = _wrn_run(False, steps)
  b = _wrn_run(True, steps)
  assert a['fired'] == b['fired'] == 6 and a['gs'] == b['gs'] == steps
  assert b['replays'] >= 10
  np.testing.assert_array_equal(a['B'], b['B'])
  np.testing.assert_array_equal(a['T'].view(np.uint32), b['T'].view(np.uint32))
  np.testing.assert_array_equal(a['W'].view(np.uint32), b['W'].view(np.uint32))
  assert (a['T'] > 0).all()


def test_checkpoint_round_trip_of_the_pruning_state(tmp_path):
  from rigl_amd import pruning, tf_checkpoint, train, variables as V
  from rigl_amd.workloads import mnist_mlp
  g = V.reset_default_graph(DEV)
  model = mnist_mlp.MnistMLP(g)
  gs = g.get_or_create_global_step()
  opt = train.MomentumOptimizer(0.05, 0.9, use_nesterov=True, graph=g)
  p = _mnist_pruning(g, gs)
  x, y = mnist_mlp.synthetic_batch(64, DEV)
  for _ in range(13):
    opt.minimize(model.loss(x, y), gs)
    p.conditional_mask_update_op()
  prefix = str(tmp_path / 'ckpt' / 'model')
  names = tf_checkpoint.save_graph(prefix, g)
  for s in ('layer1/threshold', 'layer2/threshold', 'layer3/threshold', 'model_pruning/last_mask_update_step'):
    assert s in names
  reader = tf_checkpoint.BundleReader(prefix)
  assert reader.get_tensor('model_pruning/last_mask_update_step').dtype == np.int32
  assert int(reader.get_tensor('model_pruning/last_mask_update_step')) == 12
  thr = [float(t) for t in pruning.get_thresholds(g)]
  masks = [l.mask.numpy() for l in g.masked_layers()]

  g2 = V.reset_default_graph(DEV)
  mnist_mlp.MnistMLP(g2, seed=1)
  gs2 = g2.get_or_create_global_step()
  p2 = _mnist_pruning(g2, gs2)
  loaded = tf_checkpoint.load_into_graph(prefix, g2)
  assert 'layer2/threshold' in loaded and 'model_pruning/last_mask_update_step' in loaded
  assert [float(t) for t in pruning.get_thresholds(g2)] == thr and thr[0] > 0
  for l, m in zip(g2.masked_layers(), masks):
    np.testing.assert_array_equal(l.mask.numpy(), m)
  gs2.assign(13)
  assert not p2.should_update() and int(p2._state.last_mask_update_step) == 12   # pylint: disable=protected-access
  gs2.assign(16)
  assert p2.should_update()
