"""train.MicroBatches inside a training step.  The set-up of tests/test_summary_step_gpu.py: WRN depth 10, width 1, RigL with period
5, ERK 0.8, noise_std 0; micro-batch 8.

  (a) the arena after compute_gradients(mb()) is the sequential fp32 sum of the three micro-gradients, bit for bit, and mb.loss the
      fp32 formula on the three losses;
  (b) minimize(mb(), gs) leaves the weights and slots of: that sum written into G by hand, the existing update at grad_scale 1/k
      (Nesterov momentum, and Adam); the global step advances by 1;
  (c) a mask-update call with k = 2 leaves the masks of oracle.rigl_mask_update fed the NumPy sum of the two micro-gradients;
  (d) 25 calls from a DeviceCifar with a device schedule, summaries and dropout: eager and GraphedStep(mb, ...) end bit-identical;
  (e) MicroBatches(..., 1) changes nothing, not a bit and not a launch;
  (f) the update sees a mean, not a sum: k = 4 x 32 rows against one batch of the same 128 rows on the MNIST MLP, both against an
      fp64 restatement;
  (g) misuse is refused.
"""
import types

import numpy as np
import pytest

from oracle import rigl_oracle as O

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MICRO = 8
F32 = np.float32


class _Feed:
  """loss_fn over a fixed list of micro-batches, one per call, in order."""

  def __init__(self, model, n, micro=MICRO):
    from rigl_amd.workloads import wide_resnet
    self.model = model
    self.batches = [wide_resnet.synthetic_batch(micro, DEV, seed=4321 + i) for i in range(n)]
    self.i = 0

  def __call__(self):
    x, y = self.batches[self.i % len(self.batches)]
    self.i += 1
    return self.model.loss(x, y)


def _wrn(optimizer='momentum', wrap=True, droprate=0.0, lr=0.05):
  from rigl_amd import sparse_optimizers as SO, sparse_utils, train, variables as V
  from rigl_amd.workloads import wide_resnet
  g = V.reset_default_graph(DEV)
  model = wide_resnet.WideResNet(g, depth=10, width=1, droprate=droprate)
  np.random.seed(0)
  sparse_utils.get_mask_init_fn(g.get_masks(), 'erdos_renyi_kernel', 0.8, {})()
  if optimizer == 'adam':
    inner = train.AdamOptimizer(0.001 if lr == 0.05 else lr, graph=g)
  else:
    inner = train.MomentumOptimizer(lr, 0.9, use_nesterov=True, graph=g)
  opt = SO.SparseRigLOptimizer(inner, 0, 1000, 5, drop_fraction=0.3, drop_fraction_anneal='cosine', noise_std=0.) if wrap else inner
  return g, model, inner, opt, g.get_or_create_global_step()


def _bits(t):
  return t.detach().cpu().numpy().reshape(-1).view(np.uint32).copy()


def _micro_gradients(g, inner, feed, k):
  """G and the loss after each of k single-micro-batch compute_gradients on the weights as they are."""
  Gs, Ls = [], []
  for _ in range(k):
    loss = feed()
    inner.compute_gradients(loss)
    Gs.append(g.G.cpu().numpy().copy())
    Ls.append(F32(loss.detach().cpu().item()))
  return Gs, Ls


def _seq_sum(Gs):
  s = Gs[0].copy()
  for x in Gs[1:]:
    s = (s + x).astype(F32)
  return s


# ---- (a) ---------------------------------------------------------------------------------------------------------------------
def test_a_the_arena_holds_the_sequential_fp32_sum():
  from rigl_amd import train
  g, model, inner, opt, gs = _wrn()
  feed = _Feed(model, 3)
  Gs, Ls = _micro_gradients(g, inner, feed, 3)
  assert not np.array_equal(Gs[0], Gs[1]) and not np.array_equal(Gs[1], Gs[2])      # three different micro-batches
  feed.i = 0
  mb = train.MicroBatches(feed, opt, micro_batches=3)
  loss = mb()
  gv = opt.compute_gradients(loss)                  # RigL asks the inner optimizer twice: the LAST pass runs once
  want = _seq_sum(Gs)
  np.testing.assert_array_equal(_bits(g.G), want.view(np.uint32))
  assert feed.i == 3 and len(gv) == len(g.trainable_variables())
  assert F32(loss.detach().cpu().item()) == Ls[2]                                   # the tensor returned is the k-th loss
  mean = F32(F32(F32(Ls[0] + Ls[1]) + Ls[2]) * F32(1.0 / 3))
  assert mb.loss.shape == (1,) and mb.loss.dtype == torch.float32
  assert _bits(mb.loss)[0] == np.array([mean]).view(np.uint32)[0]
  assert inner.update_scale() == 1.0 / 3
  # the second arena still holds g1 + g2: LAST only reads it
  np.testing.assert_array_equal(_bits(mb._arena), (Gs[0] + Gs[1]).astype(F32).view(np.uint32))


# ---- (b) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('optimizer', ['momentum', 'adam'])
def test_b_one_step_is_the_existing_update_of_the_sum_at_one_kth(optimizer):
  from rigl_amd import train
  k = 3
  # by hand: the summed arena written into G, the existing update at grad_scale 1 / k
  g, model, inner, _, gs = _wrn(optimizer, wrap=False)
  feed = _Feed(model, k)
  Gs, _ = _micro_gradients(g, inner, feed, k)
  g.G.copy_(torch.from_numpy(_seq_sum(Gs)))
  inner._grad_sync = types.SimpleNamespace(grad_scale=1.0 / k, enabled=False, all_reduce=lambda graph=None: None)
  inner.apply_gradients(inner._last_gv, global_step=gs)
  want = dict(W=_bits(g.W), A=_bits(inner._slot), gs=int(gs.value))
  if optimizer == 'adam':
    want['V'] = _bits(inner._slot_v)
  # accumulated
  g, model, inner, _, gs = _wrn(optimizer, wrap=False)
  feed = _Feed(model, k)
  w0 = _bits(g.W)
  mb = train.MicroBatches(feed, inner, micro_batches=k)
  inner.minimize(mb(), gs)
  assert int(gs.value) == want['gs'] == 1
  np.testing.assert_array_equal(_bits(g.W), want['W'])
  np.testing.assert_array_equal(_bits(inner._slot), want['A'])
  if optimizer == 'adam':
    np.testing.assert_array_equal(_bits(inner._slot_v), want['V'])
  assert not np.array_equal(want['W'], w0) and inner.update_scale() == 1.0       # the step moved the weights; the scale is spent


# ---- (c) ---------------------------------------------------------------------------------------------------------------------
def test_c_a_mask_update_reads_the_raw_sum():
  from rigl_amd import train
  g, model, inner, opt, gs = _wrn()
  feed = _Feed(model, 2)
  Gs, _ = _micro_gradients(g, inner, feed, 2)
  total = (Gs[0] + Gs[1]).astype(F32)
  layers = g.masked_layers()
  before = [(l.mask.numpy().copy(), l.weights.numpy().copy(), inner.get_slot(l.weights, 'momentum').cpu().numpy().copy())
            for l in layers]
  feed.i = 0
  mb = train.MicroBatches(feed, opt, micro_batches=2)
  assert opt.is_mask_update_iter(gs, opt._last_update_step)
  opt.minimize(mb(), gs)
  assert int(gs.value) == 0 and feed.i == 2                      # an update call: k micro-batches, no step
  frac = O.get_drop_fraction('cosine', 0.3, 0, 0, 1000, True)
  changed = 0
  for l, (m0, w0, a0) in zip(layers, before):
    o, n = l.weights.offset, l.weights.numel
    g0 = total[o:o + n].reshape(w0.shape)
    r = O.rigl_mask_update(m0, w0, g0, frac, momentum=a0)
    np.testing.assert_array_equal(l.mask.numpy(), r['mask'], err_msg=l.scope)
    np.testing.assert_array_equal(l.weights.numpy().view(np.uint32), r['weights'].view(np.uint32), err_msg=l.scope)
    one = O.rigl_mask_update(m0, w0, Gs[1][o:o + n].reshape(w0.shape), frac, momentum=a0)
    changed += int(np.sum(one['mask'] != r['mask']))
  assert changed > 0                                             # the last micro-gradient alone grows other connections


# ---- (d) ---------------------------------------------------------------------------------------------------------------------
CALLS = 25


def _replay_run(mode, k=2, use_mb=True, calls=CALLS):
  from rigl_amd import data, schedules as S, summaries, train
  from rigl_amd.workloads import nn as gnn
  sched = S.imagenet_lr_schedule(0.1, 32, num_train_images=40, model_architecture='mobilenet_v1')
  g, model, inner, opt, gs = _wrn(droprate=0.3, lr=sched)
  rng = np.random.RandomState(11)
  images = rng.randint(0, 256, (64, 32, 32, 3)).astype(np.uint8)
  labels = rng.randint(0, 10, 64).astype(np.int32)
  dc = data.DeviceCifar(images, labels, MICRO, seed=5, device=DEV)

  def loss_fn():
    x, y = dc.next_batch()
    return model.loss(x, y)
  fn = train.MicroBatches(loss_fn, opt, micro_batches=k) if use_mb else loss_fn
  summ = summaries.TrainingSummaries(g, opt, ring=64).attach()
  st = train.GraphedStep(fn, opt, gs, warmup=2) if mode == 'graph' else None

  def eager():
    loss = fn()
    opt.minimize(loss, gs)
    return loss
  run = st if st is not None else eager
  last, means, applied = [], [], []
  for _ in range(calls):
    s0 = int(gs.value)
    last.append(float(run().detach().float()))
    means.append(float(fn.loss) if use_mb else last[-1])
    if int(gs.value) == s0 + 1:
      applied.append((s0, means[-1]))
  torch.cuda.synchronize()
  bns = [m for m in g.modules.values() if isinstance(m, gnn.BatchNorm)]
  out = dict(W=_bits(g.W), A=_bits(inner._slot), B=g.BITS.cpu().numpy().copy(), gs=int(gs.value), last=last, means=means,
             applied=applied, position=dc.position(), stats=[_bits(t) for b in bns for t in (b.moving_mean, b.moving_variance)],
             dropout=int(model.dropout_state.step.item()))
  out['records'], out['dropped'] = summ.read(per_variable=True)
  if st is not None:
    out['replays'], out['n_graphs'] = st.replays, len(st._graphs)
  return out


_RUNS = {}


def _cached(*key, **kw):
  k = key + tuple(sorted(kw.items()))
  if k not in _RUNS:
    _RUNS[k] = _replay_run(*key, **kw)
  return _RUNS[k]


def test_d_eager_and_graphed_step_end_bit_identical():
  a, c = _cached('eager'), _cached('graph')
  for key in ('W', 'A', 'B'):
    np.testing.assert_array_equal(a[key], c[key])
  assert len(a['stats']) >= 10 and all(np.array_equal(x, y) for x, y in zip(a['stats'], c['stats']))
  assert a['last'] == c['last'] and a['means'] == c['means'] and a['gs'] == c['gs'] == CALLS - 5
  assert all(np.isfinite(a['means'])) and a['means'] != a['last']
  assert a['position'] == c['position'] == 2 * CALLS               # 64 images, 8 per micro-batch: six epoch boundaries
  assert a['dropout'] == c['dropout'] == 2 * CALLS                 # dropout draws once per micro-batch
  assert c['replays'] > 0 and c['n_graphs'] == 1
  for out in (a, c):
    assert out['dropped'] == 0
    assert [r['global_step'] for r in out['records']] == [s for s, _ in out['applied']]      # one record per applied step
    assert [r['cross_loss'] for r in out['records']] == [m for _, m in out['applied']]        # ... holding that step's mb.loss
  assert a['records'] == c['records']


# ---- (e) ---------------------------------------------------------------------------------------------------------------------
def test_e_one_micro_batch_is_free():
  from rigl_amd import ops
  a, b = _cached('eager', k=1, calls=8), _cached('eager', use_mb=False, calls=8)
  for key in ('W', 'A', 'B'):
    np.testing.assert_array_equal(a[key], b[key])
  assert a['last'] == b['last'] == a['means'] and a['records'] == b['records'] and a['position'] == b['position'] == 8
  c, d = _cached('graph', k=1, calls=8), _cached('graph', use_mb=False, calls=8)
  np.testing.assert_array_equal(c['W'], d['W'])
  np.testing.assert_array_equal(c['W'], a['W'])
  assert c['replays'] == d['replays'] > 0
  counts = []
  for use_mb in (True, False):
    from rigl_amd import train
    g, model, inner, opt, gs = _wrn(wrap=False)
    feed = _Feed(model, 1)
    fn = train.MicroBatches(feed, inner, 1) if use_mb else feed
    inner.minimize(fn(), gs)                                       # buffers and code objects settle
    torch.cuda.synchronize()
    ops.prof_enable(True)
    try:
      ops.prof_collect()
      inner.minimize(fn(), gs)
      counts.append({k: v[1] for k, v in ops.prof_collect().items()})
    finally:
      ops.prof_enable(False)
    if use_mb:
      assert fn._arena is None and fn.loss.shape == (1,)
  assert counts[0] == counts[1] and sum(counts[0].values()) > 10


# ---- (f) ---------------------------------------------------------------------------------------------------------------------
def _mlp64(g, x, y):
  """The masked MLP's gradients in fp64 on the CPU: bf16-rounded operands (inputs and mask * W), mean cross-entropy.  Returns
  {variable name: gradient}, the kernels' w.r.t. mask * W (dense)."""
  h = x.detach().cpu().double()
  leaves = {}
  layers = g.layers
  for i, l in enumerate(layers):
    w = l.weights.data.detach().cpu().float()
    if l.mask is not None:
      w = w * torch.from_numpy(l.mask.numpy().astype(np.float32)).reshape(w.shape)
    w = w.to(torch.bfloat16).double().reshape(l.weights.shape[-2], l.weights.shape[-1]).requires_grad_(True)
    bias = g.variables[l.scope + '/biases:0']
    b = bias.data.detach().cpu().double().requires_grad_(True)
    leaves[l.weights.name], leaves[bias.name] = w, b
    h = h @ w + b
    if i < len(layers) - 1:
      h = torch.relu(h)
  loss = torch.nn.functional.cross_entropy(h, y.cpu())
  loss.backward()
  return {k: v.grad.numpy().reshape(-1) for k, v in leaves.items()}


def test_f_the_update_sees_a_mean_not_a_sum():
  """Measured on an MI355X: e_acc / e_big between 0.773 and 1.016 over the six variables (profiles/accum/README.md)."""
  from rigl_amd import sparse_utils, train, variables as V
  from rigl_amd.workloads import mnist_mlp
  k, rows = 4, 32
  g = V.reset_default_graph(DEV)
  model = mnist_mlp.MnistMLP(g)
  np.random.seed(0)
  sparse_utils.get_mask_init_fn(g.get_masks(), 'random', 0.9, {'layer3': 0.0})()
  inner = train.GradientDescentOptimizer(0.1, graph=g)
  x, y = mnist_mlp.synthetic_batch(k * rows, DEV)
  G64 = _mlp64(g, x, y)
  inner.compute_gradients(model.loss(x, y))
  big = g.G.cpu().numpy().astype(np.float64)
  parts = [(x[i * rows:(i + 1) * rows].contiguous(), y[i * rows:(i + 1) * rows].contiguous()) for i in range(k)]
  it = iter(parts)
  mb = train.MicroBatches(lambda: model.loss(*next(it)), inner, micro_batches=k)
  inner.compute_gradients(mb())
  acc = g.G.cpu().numpy().astype(np.float64) / k
  assert inner.update_scale() == 1.0 / k
  assert len(G64) == 6
  for name, ref in sorted(G64.items()):
    v = g.variables[name]
    e_big = np.max(np.abs(big[v.offset:v.offset + v.numel] - ref))
    e_acc = np.max(np.abs(acc[v.offset:v.offset + v.numel] - ref))
    scale = np.max(np.abs(ref))
    print('accum (f) %-18s max|G64| %.3e  e_big %.3e  e_acc %.3e  ratio %.3f' % (name, scale, e_big, e_acc, e_acc / e_big))
    assert e_acc <= 2 * e_big, (name, e_acc, e_big)
    # ... and the bound tells a mean from a sum: the raw sum misses it (were the restatement the wrong model, e_big would be of
    # the size of the gradient itself and the sum would pass)
    assert scale > 0 and np.max(np.abs(acc[v.offset:v.offset + v.numel] * k - ref)) > 2 * e_big, name


# ---- (g) ---------------------------------------------------------------------------------------------------------------------
def test_g_misuse_is_refused():
  from rigl_amd import train
  g, model, inner, opt, gs = _wrn()
  feed = _Feed(model, 2)
  with pytest.raises(ValueError):
    train.MicroBatches(feed, opt, micro_batches=0)
  with pytest.raises(ValueError):
    train.MicroBatches(feed, opt, micro_batches=-2)
  mb = train.MicroBatches(feed, opt, micro_batches=2)
  mb()
  other = feed()
  w0 = _bits(g.W)
  with pytest.raises(RuntimeError, match='pending'):
    opt.compute_gradients(other)
  with pytest.raises(RuntimeError, match='pending'):
    inner.minimize(other, gs)
  np.testing.assert_array_equal(_bits(g.W), w0)
  assert int(gs.value) == 0
  inner._grad_sync = types.SimpleNamespace(grad_scale=0.5, enabled=True, all_reduce=lambda graph=None: None)
  with pytest.raises(NotImplementedError):
    train.MicroBatches(feed, opt, micro_batches=2)
  with pytest.raises(NotImplementedError):
    train.MicroBatches(feed, inner, micro_batches=1)
  inner._grad_sync = types.SimpleNamespace(grad_scale=1.0, enabled=False, all_reduce=lambda graph=None: None)
  train.MicroBatches(feed, opt, micro_batches=2)                   # a GradSync of one rank is no obstacle
