"""Evaluation mode on the MI355X: the frozen-batch-norm forward (``infer``), its fused kernels and the eval metrics.

* rigl_eval_metrics against a NumPy restatement of the reference's metric_fn (tf.argmax, tf.nn.in_top_k:
  imagenet_train_eval.py:596-615) -- ties at the top-1 / top-5 boundaries, +-Inf / NaN logits, labels out of range; the
  row loss must carry the bits of rigl_softmax_xent.
* the row-streaming eval epilogue (frozen bn (+ residual) (+ ReLU), optionally behind the BNL transform) must carry the bits
  of the plain forward followed by rigl_bn_apply on every ResNet-50 / MobileNet-v1 1x1 layer it takes.
* infer fused == infer unfused, bit for bit, for every workload; ResNet-50 / MobileNet-v1 logits agree with an fp32 PyTorch
  restatement (F.conv2d on mask * W, F.batch_norm(training=False)).
* evaluate() touches no state: arenas, masks, slots, moving statistics and the step are bit-unchanged, and a training run
  with an evaluation in the middle is bit-identical to one without (ResNet-50 and WRN-22, mask updates included).
"""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# fp32 restatement bound: max |infer - fp32| / max |fp32| over the logits.  Measured on an MI355X (16 images, 80 % random
# masks, random moving statistics): ResNet-50 0.0041, MobileNet-v1 0.0029 -- the bound leaves a margin of about 5x.
FP32_REL_BOUND = 0.02


# ------------------------------------------------------------------------------------------------------------------
# metrics kernel
# ------------------------------------------------------------------------------------------------------------------
def _np_metrics(z, lab, k):
  """tf.argmax (first maximum; a row with a NaN: np.argmax, the first NaN) and TF InTopK (in_topk_op.h)."""
  n, c = z.shape
  top1 = np.zeros(n, bool)
  topk = np.zeros(n, bool)
  for r in range(n):
    l = int(lab[r])
    inr = 0 <= l < c
    top1[r] = inr and int(np.argmax(z[r])) == l
    if not inr or not np.isfinite(z[r, l]) or not np.isfinite(z[r]).all():
      continue
    topk[r] = int((z[r] > z[r, l]).sum()) < k
  return top1, topk


def _np_xent(z, lab, eps):
  """Targets as tf.one_hot builds them: a label out of range has an all-zero row, t = eps / c everywhere."""
  z = z.astype(np.float64)
  c = z.shape[1]
  m = z.max(1, keepdims=True)
  lse = np.log(np.exp(z - m).sum(1, keepdims=True)) + m
  logp = z - lse
  out = np.empty(z.shape[0])
  for r in range(z.shape[0]):
    t = np.full(c, eps / c)
    if 0 <= lab[r] < c:
      t[lab[r]] += 1.0 - eps
    out[r] = -(t * logp[r]).sum()
  return out


def _metric_rows(n, c, seed):
  rs = np.random.RandomState(seed)
  z = (rs.randn(n, c) * 3).astype(np.float32)
  z = torch.from_numpy(z).to(torch.bfloat16).float().numpy()        # bf16 values: natural ties
  lab = rs.randint(0, c, n).astype(np.int64)
  # planted ties at the top-1 boundary: three maxima, the label on the first / a later one
  z[0, :] = -1.0; z[0, [3, 7, 11]] = 5.0; lab[0] = 3
  z[1, :] = -1.0; z[1, [3, 7, 11]] = 5.0; lab[1] = 7
  # ties at the top-5 boundary: four larger values, the label tied with three others at the fifth place
  z[2, :] = 0.0; z[2, [1, 2, 3, 4]] = 9.0; z[2, [5, 6, 7, 8]] = 4.0; lab[2] = 6
  # five strictly larger: miss
  z[3, :] = 0.0; z[3, [1, 2, 3, 4, 5]] = 9.0; z[3, 6] = 4.0; lab[3] = 6
  # non-finite logits: +Inf elsewhere, -Inf on the label, NaN elsewhere, NaN on the label, +Inf on the label
  z[4, 9] = np.inf
  z[5, lab[5]] = -np.inf
  z[6, 2] = np.nan
  z[7, lab[7]] = np.nan
  z[8, lab[8]] = np.inf
  z[9, 1] = np.nan; z[9, 4] = np.nan                               # two NaNs: np.argmax takes the first
  lab[9] = 1
  # labels out of range
  lab[10] = -1
  lab[11] = c
  # the label is the row's maximum
  lab[12] = int(np.argmax(z[12]))
  return z, lab


@pytest.mark.parametrize('c', [1000, 16])
@pytest.mark.parametrize('eps', [0.0, 0.1])
def test_eval_metrics_kernel_matches_metric_fn(c, eps):
  from rigl_amd import ops
  n = 37
  z, lab = _metric_rows(n, c, c + int(eps * 10))
  zt = torch.from_numpy(z).to(torch.bfloat16).to(DEV)
  lt = torch.from_numpy(lab).to(DEV)
  for k in range(1, 6):
    counts = torch.zeros(3, dtype=torch.int64, device=DEV)
    loss, flags = ops.eval_metrics(zt, lt, eps, k, counts=counts)
    ref_loss, _ = ops.softmax_xent(zt, lt, eps, want_grad=False)
    torch.cuda.synchronize()
    assert torch.equal(loss.view(torch.int32), ref_loss.view(torch.int32)), 'row loss: not the bits of rigl_softmax_xent'
    f = flags.cpu().numpy()
    t1, tk = _np_metrics(z, lab, k)
    np.testing.assert_array_equal(f & 1, t1.astype(np.int32), err_msg='top-1, k=%d' % k)
    np.testing.assert_array_equal((f >> 1) & 1, tk.astype(np.int32), err_msg='top-%d' % k)
    assert counts.cpu().tolist() == [n, int(t1.sum()), int(tk.sum())]
    if k == 5:
      assert tk[2] and not tk[3] and t1[0] and not t1[1] and not tk[4] and not tk[7] and not t1[10] and not tk[11]
      assert t1[9] == (lab[9] == 1)
  fin = np.isfinite(z).all(1)                     # labels out of range included: the smoothing term alone (tf.one_hot)
  assert not ((lab[fin] >= 0) & (lab[fin] < c)).all()
  np.testing.assert_allclose(loss.cpu().numpy()[fin], _np_xent(z, lab, eps)[fin], rtol=2e-5, atol=1e-5)


def test_bn_infer_params_is_the_finalize_algebra():
  from rigl_amd import ops

  class _V:
    def __init__(self, t):
      self.data = t

  class _B:
    pass
  bns = []
  rs = np.random.RandomState(3)
  for c in (64, 2048, 8, 520):
    b = _B()
    b.gamma = _V(torch.from_numpy((rs.rand(c) + 0.5).astype(np.float32)).to(DEV))
    b.beta = _V(torch.from_numpy(rs.randn(c).astype(np.float32)).to(DEV))
    b.moving_mean = torch.from_numpy(rs.randn(c).astype(np.float32)).to(DEV)
    b.moving_variance = torch.from_numpy((rs.rand(c) * 2).astype(np.float32)).to(DEV)
    b.eps = 1e-5 if c != 8 else 1e-3
    bns.append(b)
  bns = bns * 20                                          # 80 items: two launches of the batched kernel
  out = ops.bn_infer_params(bns)
  torch.cuda.synchronize()
  for b, o in zip(bns, out):
    g, be = b.gamma.data.cpu().numpy(), b.beta.data.cpu().numpy()
    mm, mv = b.moving_mean.cpu().numpy(), b.moving_variance.cpu().numpy()
    invstd = (1.0 / np.sqrt(mv.astype(np.float64) + np.float64(np.float32(b.eps)))).astype(np.float32)
    sc = (g * invstd).astype(np.float32)
    sh = (be - (mm * sc).astype(np.float32)).astype(np.float32)
    np.testing.assert_array_equal(o[0].cpu().numpy().view(np.uint32), sc.view(np.uint32))
    np.testing.assert_array_equal(o[1].cpu().numpy().view(np.uint32), sh.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------
# row-streaming eval epilogue
# ------------------------------------------------------------------------------------------------------------------
# (h, cin, cout) of the 1x1 / stride-1 layers: ResNet-50 (resnet_model.py:396-501) and MobileNet-v1 pointwise
# (mobilenetv1_model.py:156-342)
RESNET_1X1 = ((56, 64, 64), (56, 64, 256), (56, 256, 64), (28, 256, 128), (28, 128, 512), (28, 512, 128), (14, 512, 256),
              (14, 256, 1024), (14, 1024, 256), (7, 1024, 512), (7, 512, 2048), (7, 2048, 512))
MOBILENET_1X1 = ((112, 32, 64), (56, 64, 128), (56, 128, 128), (28, 128, 256), (28, 256, 256), (14, 256, 512),
                 (14, 512, 512), (7, 512, 1024), (7, 1024, 1024))


def _ss(c, gen, scale=1.0):
  return torch.stack([torch.rand(c, device=DEV, generator=gen) * scale + 0.25,
                      torch.randn(c, device=DEV, generator=gen) * 0.5])


def _check_layer(n, h, ci, co, seed):
  """Returns how many forms ran fused; asserts every form carries the bits of the separate passes."""
  from rigl_amd import ops
  d = ops.conv_desc(n, h, h, ci, co, 1, 1, 1, 0, 0, h, h)
  gen = torch.Generator(device=DEV).manual_seed(seed)
  x = (torch.randn(n, h, h, ci, device=DEV, generator=gen) * 1.5 + 0.2).to(torch.bfloat16)
  w = (torch.randn(ci * co, device=DEV, generator=gen) * (2.0 / ci) ** 0.5).to(torch.bfloat16)
  ss, ss_in = _ss(co, gen), _ss(ci, gen)
  res = torch.randn(n, h, h, co, device=DEV, generator=gen).to(torch.bfloat16)
  fused = 0
  plain = ops.conv_fwd(d, x, w)
  for relu in (False, True):
    for r in (None, res):
      if ops.conv_fwd_takes_bn_epilogue(d, False, r is not None):
        fused += 1
      y = ops.conv_fwd(d, x, w, scale_shift=ss, residual=r, relu=relu)
      y_ref = ops.bn_apply(plain, ss, relu=relu, residual=r)
      assert torch.equal(y.view(torch.int16), y_ref.view(torch.int16)), (h, ci, co, relu, r is not None)
  a = ops.bn_apply(x, ss_in, relu=True)
  plain_a = ops.conv_fwd(d, a, w)
  if ops.conv_fwd_takes_bn_epilogue(d, True):
    fused += 1
  y = ops.conv_fwd_bnrelu(d, x, ss_in, w, None)
  assert torch.equal(y.view(torch.int16), plain_a.view(torch.int16)), ('bnl', h, ci, co)
  for relu in (False, True):
    for r in (None, res):
      if ops.conv_fwd_takes_bn_epilogue(d, True, r is not None):
        fused += 1
      y = ops.conv_fwd_bnrelu(d, x, ss_in, w, None, scale_shift=ss, residual=r, relu=relu)
      y_ref = ops.bn_apply(plain_a, ss, relu=relu, residual=r)
      assert torch.equal(y.view(torch.int16), y_ref.view(torch.int16)), ('bnl', h, ci, co, relu, r is not None)
  assert float(y_ref.float().abs().max()) > 0 and (y_ref == 0).any()
  return fused


@pytest.mark.parametrize('net', ['resnet50', 'mobilenet_v1'])
def test_rowstream_eval_epilogue_is_conv_then_apply(net):
  from rigl_amd import ops
  shapes = RESNET_1X1 if net == 'resnet50' else MOBILENET_1X1
  fused, taken = 0, 0
  for i, (h, ci, co) in enumerate(shapes):
    d = ops.conv_desc(128, h, h, ci, co, 1, 1, 1, 0, 0, h, h)
    if not ops.conv_fwd_takes_bn_epilogue(d):
      continue
    taken += 1
    fused += _check_layer(128, h, ci, co, 100 + i)
  assert taken >= 4 and fused >= 4 * taken, (taken, fused)


def test_rowstream_eval_epilogue_ragged_rows():
  from rigl_amd import ops
  ops.tune_set('rowstream', 2)
  try:
    for (h, ci, co) in ((28, 128, 512), (28, 512, 128), (28, 64, 256), (28, 128, 64)):
      d = ops.conv_desc(7, h, h, ci, co, 1, 1, 1, 0, 0, h, h)         # 5 488 rows: the last fragments are partial
      assert ops.conv_fwd_takes_bn_epilogue(d)
      assert _check_layer(7, h, ci, co, 7 + ci) >= 4
  finally:
    ops.tune_unset('rowstream')


def test_eval_fuse_knob_off_takes_nothing():
  from rigl_amd import ops
  d = ops.conv_desc(128, 28, 28, 128, 512, 1, 1, 1, 0, 0, 28, 28)
  assert ops.conv_fwd_takes_bn_epilogue(d)
  ops.tune_set('eval_fuse', 0)
  try:
    assert not ops.conv_fwd_takes_bn_epilogue(d) and not ops.conv_fwd_takes_bn_epilogue(d, True)
  finally:
    ops.tune_unset('eval_fuse')


# ------------------------------------------------------------------------------------------------------------------
# whole models
# ------------------------------------------------------------------------------------------------------------------
def _randomise(g, seed, sparsity=0.0):
  from rigl_amd import sparse_utils
  from rigl_amd.workloads import nn as gnn
  gen = torch.Generator(device=DEV).manual_seed(seed)
  for m in g.modules.values():
    if isinstance(m, gnn.BatchNorm):
      c = m.channels
      m.gamma.data.copy_(torch.rand(c, device=DEV, generator=gen) * 0.5 + 0.5)
      m.beta.data.copy_(torch.randn(c, device=DEV, generator=gen) * 0.1)
      m.moving_mean.copy_(torch.randn(c, device=DEV, generator=gen) * 0.1)
      m.moving_variance.copy_(torch.rand(c, device=DEV, generator=gen) + 0.5)
  if sparsity:
    np.random.seed(seed)
    sparse_utils.get_mask_init_fn(g.get_masks(), 'random', sparsity, {})()
  g.shadows_dirty = True


def _build(name, seed=0):
  from rigl_amd import variables as V
  from rigl_amd.workloads import mnist_mlp, mobilenet_v1, resnet50, wide_resnet
  g = V.reset_default_graph(DEV)
  if name == 'resnet50':
    m = resnet50.ResNet50(g, seed=seed)
    x, y = resnet50.synthetic_batch(128, DEV)
  elif name == 'mobilenet_v1':
    m = mobilenet_v1.MobileNetV1(g, seed=seed)
    x, y = mobilenet_v1.synthetic_batch(128, DEV)
  elif name == 'wrn22':
    m = wide_resnet.WideResNet(g, depth=22, seed=seed)
    x, y = wide_resnet.synthetic_batch(64, DEV)
  else:
    m = mnist_mlp.MnistMLP(g, seed=seed)
    x, y = mnist_mlp.synthetic_batch(64, DEV)
  return g, m, x, y


@pytest.mark.parametrize('name', ['resnet50', 'mobilenet_v1'])
def test_infer_fused_equals_unfused(name):
  """(WRN-22 and MNIST have no fused form: their infer runs the same kernels either way -- test_infer_agrees_with_... below.)"""
  from rigl_amd import ops
  g, m, x, _ = _build(name)
  _randomise(g, 5, 0.8 if name != 'mnist' else 0.0)
  a = m.infer(x)
  ops.tune_set('eval_fuse', 0)
  try:
    b = m.infer(x)
  finally:
    ops.tune_unset('eval_fuse')
  torch.cuda.synchronize()
  assert a.dtype == torch.float32 and a.shape == (x.shape[0], 1000)
  assert torch.isfinite(a).all() and float(a.std()) > 0
  assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# max |infer - model(x, is_training=False)| / max |model(x, is_training=False)| (the training modules in eval mode: F.batch_norm on
# the bf16 tensors, another rounding of the same frozen batch norm).  Measured on an MI355X (32 images, 80 % random masks,
# random moving statistics): ResNet-50 0.0050, MobileNet-v1 0.0037, WRN-22 0.0114 -- the bound leaves a margin of 3.5x or more.
TRAIN_EVAL_BOUND = 0.04


@pytest.mark.parametrize('name', ['resnet50', 'mobilenet_v1', 'wrn22', 'mnist'])
def test_infer_agrees_with_the_training_modules_in_eval_mode(name):
  """An independent check of each infer()'s dataflow: the workload's own __call__ with is_training=False (MNIST has no batch
  norm: the same kernels, the same bits)."""
  g, m, x, _ = _build(name)
  _randomise(g, 17, 0.8 if name != 'mnist' else 0.0)
  x = x[:32].contiguous()
  a = m.infer(x)
  with torch.no_grad():
    ref = (m(x) if name == 'mnist' else m(x, is_training=False)).float()
  torch.cuda.synchronize()
  if name == 'mnist':
    assert torch.equal(a.view(torch.int32), ref.view(torch.int32))
    return
  rel = float((a - ref).abs().max() / ref.abs().max())
  print('%s: max |infer - eval-mode modules| / max = %.4g' % (name, rel))
  assert float(ref.std()) > 0
  assert rel < TRAIN_EVAL_BOUND, rel


def _w(conv):
  lv = conv.vars
  w = lv.weights.data
  if lv.mask is not None:
    w = w * lv.mask.data.to(w.dtype)
  return w


def _conv32(conv, x, stride, pad):
  return torch.nn.functional.conv2d(x, _w(conv).permute(3, 2, 0, 1), stride=stride, padding=pad)


def _bn32(bn, x, relu=True, res=None):
  y = torch.nn.functional.batch_norm(x, bn.moving_mean, bn.moving_variance, bn.gamma.data, bn.beta.data, False, 0.0, bn.eps)
  if res is not None:
    y = y + res
  return torch.relu(y) if relu else y


def _resnet32(m, images):
  F = torch.nn.functional
  x = images.float().permute(0, 3, 1, 2)
  x = _bn32(m.stem_bn, _conv32(m.stem.conv, x, 2, 3))
  x = F.max_pool2d(F.pad(x, (0, 1, 0, 1), value=float('-inf')), 3, 2)        # TF SAME on an even size: bottom / right
  for b in m.blocks:
    y = _bn32(b.bn1, _conv32(b.c1.conv, x, 1, 0))
    y = _bn32(b.bn2, _conv32(b.c2.conv, y, b.c2.stride, 1))
    s = _bn32(b.proj_bn, _conv32(b.proj.conv, x, b.proj.stride, 0), relu=False) if b.proj is not None else x
    x = _bn32(b.bn3, _conv32(b.c3.conv, y, 1, 0), res=s)
  x = x.mean(dim=(2, 3))
  return x @ _w(m.fc) + m.fc.bias.data


def _mobilenet32(m, images):
  F = torch.nn.functional
  x = images.float().permute(0, 3, 1, 2)
  x = _bn32(m.stem_bn, _conv32(m.stem, x, 2, 1))
  for dw, bn_a, pw, bn_b in m.blocks:
    wd = dw.weights.data.permute(2, 3, 0, 1)                                  # (3, 3, C, 1) -> (C, 1, 3, 3)
    x = _bn32(bn_a, F.conv2d(x, wd, stride=dw.stride, padding=1, groups=dw.channels))
    x = _bn32(bn_b, _conv32(pw, x, 1, 0))
  x = x.mean(dim=(2, 3))
  return x @ _w(m.fc) + m.fc.bias.data


@pytest.mark.parametrize('name', ['resnet50', 'mobilenet_v1'])
def test_infer_agrees_with_an_fp32_restatement(name, record_property):
  g, m, x, _ = _build(name)
  _randomise(g, 9, 0.8)
  x = x[:16].contiguous()
  a = m.infer(x)
  with torch.no_grad():
    ref = (_resnet32 if name == 'resnet50' else _mobilenet32)(m, x)
  torch.cuda.synchronize()
  rel = float((a - ref).abs().max() / ref.abs().max())
  record_property('fp32_rel_err', rel)
  print('%s: max |infer - fp32| / max |fp32| = %.4g' % (name, rel))
  assert float(ref.std()) > 0
  assert rel < FP32_REL_BOUND, rel
  # the top-1 decisions agree where the fp32 margin is clear
  srt = ref.sort(dim=1, descending=True).values
  clear = (srt[:, 0] - srt[:, 1]) > 4 * float((a - ref).abs().max())
  assert torch.equal(a.argmax(1)[clear], ref.argmax(1)[clear])


# ------------------------------------------------------------------------------------------------------------------
# no side effects
# ------------------------------------------------------------------------------------------------------------------
def _state(g, inner=None):
  from rigl_amd.workloads import nn as gnn
  out = dict(W=g.W.clone(), B=g.BITS.clone(), gs=int(g.global_step.value) if g.global_step is not None else None)
  if inner is not None and getattr(inner, '_slot', None) is not None:
    out['A'] = inner._slot.clone()
  out['stats'] = [t.clone() for m in g.modules.values() if isinstance(m, gnn.BatchNorm) for t in (m.moving_mean, m.moving_variance)]
  return out


def _same(a, b):
  assert a['gs'] == b['gs']
  assert torch.equal(a['W'].view(torch.int32), b['W'].view(torch.int32))
  assert torch.equal(a['B'], b['B'])
  if 'A' in a or 'A' in b:
    assert torch.equal(a['A'].view(torch.int32), b['A'].view(torch.int32))
  assert len(a['stats']) == len(b['stats'])
  for s, t in zip(a['stats'], b['stats']):
    assert torch.equal(s.view(torch.int32), t.view(torch.int32))


def test_evaluate_touches_no_state_and_batch_statistics_update_nothing():
  from rigl_amd import evaluation as E
  g, m, x, y = _build('mobilenet_v1')
  _randomise(g, 11, 0.5)
  g.get_or_create_global_step()
  before = _state(g)
  r = E.evaluate(m, [(x[:40], y[:40]), (x[40:64], y[40:64])], eval_once=True)
  torch.cuda.synchronize()
  _same(before, _state(g))
  r2 = E.evaluate(m, [(x[:40], y[:40])], use_batch_statistics=True)
  torch.cuda.synchronize()
  _same(before, _state(g))
  for v in list(r.values()) + list(r2.values()):
    assert np.isfinite(v)


def test_resnet50_batch_statistics_update_nothing():
  """use_batch_statistics on ResNet-50: the stem tail (rigl_bn_relu_maxpool_fwd), the pair kernel (rigl_bn_add_bn_fwd) and the
  plain batch norms all run with the moving-statistics pointers NULL."""
  from rigl_amd import evaluation as E, variables as V
  from rigl_amd.workloads import resnet50
  g = V.reset_default_graph(DEV)
  m = resnet50.ResNet50(g)
  x, y = resnet50.synthetic_batch(8, DEV, image_size=64)
  _randomise(g, 19, 0.8)
  before = _state(g)
  r = E.evaluate(m, [(x, y)], use_batch_statistics=True)
  torch.cuda.synchronize()
  _same(before, _state(g))
  assert all(np.isfinite(v) for v in r.values())
  assert r['cross_loss'] != E.evaluate(m, [(x, y)])['cross_loss']       # the batch's own statistics, not the moving ones


def _train_run(name, evaluate_at, steps, graphed=False, depth=22, period=3):
  """``steps`` training calls (eager, or train.GraphedStep) with evaluate() before call ``evaluate_at``; returns the final state
  (and, graphed, the replays before / after the evaluation)."""
  from rigl_amd import evaluation as E, sparse_optimizers as SO, sparse_utils, train, variables as V
  from rigl_amd.workloads import resnet50, wide_resnet
  g = V.reset_default_graph(DEV)
  if name == 'resnet50':
    m = resnet50.ResNet50(g)
    x, y = resnet50.synthetic_batch(8, DEV, image_size=64)
  else:
    m = wide_resnet.WideResNet(g, depth=depth)
    x, y = wide_resnet.synthetic_batch(32, DEV)
  np.random.seed(0)
  sparse_utils.get_mask_init_fn(g.get_masks(), 'erdos_renyi_kernel', 0.8, {})()
  inner = train.MomentumOptimizer(0.05, 0.9, use_nesterov=True, graph=g)
  opt = SO.SparseRigLOptimizer(inner, 0, 1000, period, drop_fraction=0.3, drop_fraction_anneal='cosine', noise_std=0.)
  gs = g.get_or_create_global_step()
  st = train.GraphedStep(lambda: m.loss(x, y), opt, gs, warmup=2) if graphed else None

  def run():
    if st is not None:
      st()
    else:
      opt.minimize(m.loss(x, y), gs)
  replays_before = 0
  for i in range(steps):
    if i == evaluate_at:
      torch.cuda.synchronize()
      before = _state(g, inner)
      replays_before = st.replays if st is not None else 0
      E.evaluate(m, [(x, y)], eval_once=True)
      torch.cuda.synchronize()
      _same(before, _state(g, inner))
    run()
  torch.cuda.synchronize()
  out = _state(g, inner)
  if st is not None:
    out['replays'] = (replays_before, st.replays - replays_before)
  return out


def test_resnet50_step_evaluate_step_equals_step_step():
  a = _train_run('resnet50', 1, 5)          # calls 0 and 4 update the masks (period 3: an update does not advance the step)
  b = _train_run('resnet50', -1, 5)
  _same(a, b)


def test_wrn22_step_evaluate_step_equals_step_step():
  a = _train_run('wrn22', 2, 6)
  b = _train_run('wrn22', -1, 6)
  _same(a, b)


def test_wrn_graphed_step_evaluate_step_equals_step_step():
  """train_and_eval under graph replay: an evaluation between replayed steps changes nothing the captured graph reads.  The
  WRN of tests/test_graphed_step_gpu.py (depth 10, mask period 5: calls 0, 6, 12, 18 update the masks eagerly).  WRN-22 at
  batch 32 is not used: its first capture faults in torch.cuda.graph's capture_end in a process that never evaluates (the
  training step alone; see the reply to the review of the eval path)."""
  a = _train_run('wrn', 9, 19, graphed=True, depth=10, period=5)
  b = _train_run('wrn', -1, 19, graphed=True, depth=10, period=5)
  assert a['replays'][0] >= 3 and a['replays'][1] >= 3, a['replays']     # replays before and after the evaluation
  _same(a, b)


# ------------------------------------------------------------------------------------------------------------------
# evaluate() end to end
# ------------------------------------------------------------------------------------------------------------------
def test_evaluate_end_to_end_and_checkpoint_round_trip(tmp_path):
  from rigl_amd import evaluation as E, tf_checkpoint, variables as V
  from rigl_amd.workloads import wide_resnet
  g, m, x, y = _build('wrn22')
  _randomise(g, 13, 0.7)
  batches = [(x[:32], y[:32]), (x[32:51], y[32:51]), (x[51:64], y[51:64])]        # the last of uneven size
  r = E.evaluate(m, batches, label_smoothing=0.1, eval_once=True, chunk=16)
  logits = torch.cat([m.infer(b[0]) for b in batches]).to(torch.bfloat16).float().cpu().numpy()
  lab = y[:64].cpu().numpy()
  t1, t5 = _np_metrics(logits, lab, 5)
  assert r['eval_accuracy'] == pytest.approx(t1.mean(), abs=1e-12)
  assert r['top_5_eval_accuracy'] == pytest.approx(t5.mean(), abs=1e-12)
  assert r['cross_loss'] == pytest.approx(_np_xent(logits, lab, 0.1).mean(), rel=1e-5)
  want = 0.0
  for v in g.variables.values():
    if getattr(v, 'weight_decay', 0.0) > 0.0:
      w = v.data.cpu().numpy().astype(np.float64)
      want += v.weight_decay * (w * w).sum() / 2.0
  assert r['reg_loss'] == pytest.approx(want, rel=1e-12)
  sp = {k: v for k, v in r.items() if k.startswith('pruning/')}
  assert len(sp) == len(g.get_masks()) and set(r) == set(E.METRIC_KEYS) | set(sp)
  for mk in g.get_masks():
    assert sp['pruning/%s/sparsity' % mk.name[:-2]] == pytest.approx(1.0 - mk.sum() / mk.numel, abs=1e-12)
  assert E.metric_fn(torch.from_numpy(lab).to(DEV), torch.from_numpy(logits).to(DEV), 0.5, 0.25)['eval_accuracy'] == \
      pytest.approx(t1.mean(), abs=1e-12)
  # save, restore into a fresh model, infer: the same bits
  a = m.infer(x)
  prefix = str(tmp_path / 'model.ckpt-0')
  tf_checkpoint.save_graph(prefix, g)
  g2 = V.reset_default_graph(DEV)
  m2 = wide_resnet.WideResNet(g2, depth=22, seed=7)
  tf_checkpoint.load_into_graph(prefix, g2, strict=True)
  b = m2.infer(x)
  torch.cuda.synchronize()
  assert torch.equal(a.view(torch.int32), b.view(torch.int32))
