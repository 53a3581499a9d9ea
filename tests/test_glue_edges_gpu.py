"""The glue kernels -- max pool, fused stem tail, softmax cross-entropy, global average pool, the batched packers -- held
to the plain float64 references of tests/glue_ref.py at the shapes and inputs where such kernels go wrong.

Everything compared against is computed in this process on the CPU (tests/glue_ref.py, oracle/); no vendor kernel is a
reference here.  Each tolerance is derived, not measured, and tests/test_glue_ref_cpu.py shows on the same inputs that
an fp32 restatement of each documented formula stays inside half of it.  Every test prints its worst figure before it
asserts.

Outside the pinned contract: a pooling window that holds nothing but -inf (the kernel reports tap 0, the reference the
first in-image tap), NaN inputs anywhere, and non-finite logits.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip('torch')

from tests import convref, glue_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL16 = 0x7FA5                       # a bf16 NaN no kernel here produces
SENTINEL32 = 0x7FA5A5A5


def _bits(t):
  return t.detach().cpu().contiguous().view(torch.int16)


def _sentinel_bf16(shape):
  return torch.full(shape, SENTINEL16, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def _gdesc(d):
  from rigl_amd import ops
  return ops.conv_desc(d.n, d.h, d.w, d.cin, d.cin, d.kh, d.kw, (d.stride_h, d.stride_w), d.pad_top, d.pad_left, d.ho, d.wo)


def _ptr(t):
  return C.c_void_p(t.data_ptr())


# ---------------------------------------------------------------------------------------------------------------------
# max pooling
# ---------------------------------------------------------------------------------------------------------------------
def _check_maxpool(name, d, x, dy):
  """y and argmax bit-identical to the reference; dx (written into a sentinel-filled buffer) within the project's bound,
  bit-identical where at most one window names the pixel, exactly zero where none does.  Returns the worst dx ratio."""
  from rigl_amd import _lib, ops
  gd = _gdesc(d)
  y, arg = ops.maxpool_fwd(gd, x.to(DEV))
  yr, ar = R.maxpool_ref(x, d)
  assert torch.equal(_bits(y), _bits(yr)), '%s: y is not the bits of the first maximum' % name
  assert torch.equal(arg.cpu(), ar), '%s: argmax is not r * kw + s of the first maximum' % name
  dxr, ab, cnt = R.maxpool_bwd_ref(dy, ar, d)
  dyg = dy.to(DEV)
  dx = _sentinel_bf16((d.n, d.h, d.w, d.cin))
  _lib.check(_lib.load().rigl_maxpool_bwd(C.byref(gd), _ptr(dyg), _ptr(arg), _ptr(dx), ops._stream()))
  assert torch.equal(_bits(ops.maxpool_bwd(gd, dyg, arg)), _bits(dx))
  dxc = dx.cpu()
  assert not (_bits(dxc) == SENTINEL16).any(), '%s: dx elements never written' % name
  ratio = convref.check_close(name + ' dx', dxc.float(), dxr, ab, rel=1e-5, out_ulp=2.0**-8)
  one = cnt <= 1
  assert torch.equal(_bits(dxc)[one], _bits(dxr.to(torch.bfloat16))[one]), '%s: dx of a single window is not its dy' % name
  assert (_bits(dxc)[cnt == 0] == 0).all(), '%s: dx is not +0 where no window names the pixel' % name
  return ratio


GEOMS = R.small_pool_geometries()


@pytest.mark.parametrize('name,d', GEOMS, ids=[g[0] for g in GEOMS])
def test_maxpool_matches_the_first_maximum_reference(name, d):
  worst = 0.0
  for i, kind in enumerate(R.POOL_INPUT_KINDS):
    worst = max(worst, _check_maxpool('%s %s' % (name, kind), d, R.pool_input(kind, d, 100 + i), R.pool_dy(d, 100 + i)))
  print('%s: worst dx error / bound %.3g' % (name, worst))
  if (d.kh, d.kw, d.stride_h, d.stride_w) == (2, 2, 2, 2):
    _, _, cnt = R.maxpool_bwd_ref(R.pool_dy(d, 0), R.maxpool_ref(R.pool_input('normal', d, 0), d)[1], d)
    assert int(cnt.max()) == 1                              # 2x2 / 2: every comparison above was bit for bit


@pytest.mark.parametrize('name,d', [('stem_128x112x112x64_3x3s2_same', R.same_pool_desc(128, 112, 112, 64, 3, 2)),
                                    ('vgg16_128x56x56x256_2x2s2', R.valid_pool_desc(128, 56, 56, 256, 2, 2))],
                         ids=['resnet50_stem', 'vgg16_pool'])
def test_maxpool_benchmarked_tensors(name, d):
  """The two full-size tensors, once each (bf16 normals tie often), outside the input sweep.  Measured: worst dx error
  / bound 0.994 on the stem (the bf16 store of a sum of up to four terms), 0 on the 2x2 / 2 pool (bit for bit)."""
  ratio = _check_maxpool(name, d, R.pool_input('normal', d, 1), R.pool_dy(d, 1))
  print('%s: worst dx error / bound %.3g' % (name, ratio))


@pytest.mark.parametrize('name,d', GEOMS, ids=[g[0] for g in GEOMS])
def test_fused_stem_tail_matches_bn_relu_then_the_reference_pool(name, d):
  """rigl_bn_relu_maxpool_fwd (the kernel behind ops.bn_relu_maxpool_fwd, called with a given scale / shift: the wrapper
  derives them from batch statistics) and ops.bn_relu_maxpool_infer against maxpool_ref(bf16(relu(fma(x, scale, shift)))):
  identity parameters, and parameters that send whole windows to +0 (ties over every in-image tap)."""
  from rigl_amd import _lib, ops
  gd = _gdesc(d)
  lib = _lib.load()
  for which in ('identity', 'zeros'):
    scale, shift = R.bn_relu_params(d.cin, which)
    ss = torch.stack([scale, shift]).to(DEV)
    for i, kind in enumerate(R.POOL_INPUT_KINDS):
      x = R.pool_input(kind, d, 100 + i)
      yr, ar = R.maxpool_ref(R.bn_relu_ref(x, scale, shift), d)
      xg = x.to(DEV)
      y = _sentinel_bf16((d.n, d.ho, d.wo, d.cin))
      arg = torch.full((d.n, d.ho, d.wo, d.cin), 0xEE, dtype=torch.uint8, device=DEV)
      _lib.check(lib.rigl_bn_relu_maxpool_fwd(C.byref(gd), _ptr(xg), _ptr(ss[0]), _ptr(ss[1]), _ptr(y), _ptr(arg), ops._stream()))
      what = '%s %s %s' % (name, which, kind)
      assert torch.equal(_bits(y), _bits(yr)), what + ': y'
      assert torch.equal(arg.cpu(), ar), what + ': argmax'
      assert torch.equal(_bits(ops.bn_relu_maxpool_infer(gd, xg, ss)), _bits(yr)), what + ': infer y'
      if which == 'zeros' and kind == 'normal':
        assert float((yr == 0).float().mean()) > 0.2        # whole windows did tie at +0


def test_fused_stem_tail_through_its_wrapper():
  """ops.bn_relu_maxpool_fwd end to end: the scale / shift it derived from the batch go into the reference."""
  from rigl_amd import ops
  d = R.same_pool_desc(4, 18, 14, 64, 3, 2)
  x = R.pool_input('normal', d, 11)
  g = torch.Generator().manual_seed(11)
  gamma = (torch.rand(d.cin, generator=g) + 0.5).to(DEV)
  beta = (torch.randn(d.cin, generator=g) - 1.0).to(DEV)
  rm, rv = torch.zeros(d.cin, device=DEV), torch.ones(d.cin, device=DEV)
  y, arg, saved = ops.bn_relu_maxpool_fwd(_gdesc(d), x.to(DEV), gamma, beta, rm, rv, 0.9, 1e-5)
  yr, ar = R.maxpool_ref(R.bn_relu_ref(x, saved[2].cpu(), saved[3].cpu()), d)
  assert torch.equal(_bits(y), _bits(yr)) and torch.equal(arg.cpu(), ar)
  assert (yr == 0).any() and (yr != 0).any()


# ---------------------------------------------------------------------------------------------------------------------
# softmax cross-entropy
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', R.XENT_K)
def test_softmax_xent_matches_the_float64_reference(k):
  """Per row and per element, in the project's "1e-5 of the magnitudes of the terms" form (tests/glue_ref.xent_ref):
    loss     |got - ref| <= 1e-5 * (on * (lse + |z_lab - m|) + off * (K * lse + sum_k |z_k - m|)) + 1e-6
    gradient |got - ref| <= 2^-8 |ref| + 1e-5 * |grad_scale| * (p * max(1, |z - m - lse|) + t)
  with tf.one_hot targets: a label outside [0, K) leaves the smoothing term alone (no `on` term in loss or gradient).
  In-range rows: the float64 sum of the stored dlogits is zero to within K bf16 half ulps of the row's largest entry
  (rows whose entries are all below 2^-12 |grad_scale| get the fp32 allowance instead: glue_ref.xent_row_sum_rows).
  The row loss of ops.eval_metrics must carry the same bits (K <= 8192).  The offset logits are randn * 8 +- 200, not
  randn * 40 +- 200: glue_ref.XENT_SPREAD says why (fp32 restatement, K = 20 000, eps 0: gradient error 114 times the
  bound at spread 16 or 40 -- got 0, ref e^-110 and smaller -- and 0.98 of it at spread 8).
  Measured on an MI355X, worst error / bound over the sweep: loss 0.59 (K = 20 000; 0.31 or less elsewhere), gradient
  0.94 - 0.99 (the bf16 store's half ulp just above a power of two, which the 2^-8 |ref| term is), row sum 1.0 at K = 2
  (two entries of one magnitude rounded in opposite directions), 0.3 at K = 10 and below 0.11 from K = 37 on.  Before
  the out-of-range fix of head.hip: all-equal logits with label -1, eps 0 gave loss log K against a reference of 0 (error
  7e5 .. 1e7 times the bound) for every K above 1."""
  from rigl_amd import ops
  worst = [0.0, 0.0, 0.0]
  for rows, seed, eps, gs in R.xent_sweep(k):
    z, lab = R.xent_inputs(rows, k, seed)
    ref = R.xent_ref(z, lab, eps, gs)
    zg, lg = z.to(DEV), lab.to(DEV)
    loss, dz = ops.softmax_xent(zg, lg, eps, grad_scale=gs)
    what = 'K=%d rows=%d seed=%d eps=%g scale=%g' % (k, rows, seed, eps, gs)
    if k <= R.XENT_EVAL_MAX_K:
      eloss, _ = ops.eval_metrics(zg, lg, eps, 5)
      assert torch.equal(eloss.view(torch.int32), loss.view(torch.int32)), what + ': eval_metrics row loss: other bits'
    loss, dz = loss.cpu().double(), dz.cpu()
    rl = (loss - ref.loss).abs() / ref.loss_bound
    rg = (dz.double() - ref.dlogits).abs() / ref.grad_bound
    strict = R.xent_row_sum_rows(ref, lab, gs)
    loose = (lab >= 0) & (lab < k) & ~strict
    rsum = dz.double().sum(dim=1).abs()
    rs = torch.where(strict, rsum / R.xent_row_sum_bound(dz, k), torch.zeros((), dtype=torch.float64))
    rs = torch.where(loose, rsum / R.xent_row_sum_fp32_bound(ref, dz).clamp(min=1e-300), rs)
    worst = [max(a, float(b.max())) for a, b in zip(worst, (rl, rg, rs))]
    i = int(rl.argmax())
    assert float(rl.max()) <= 1.0, '%s: row %d label %d loss %r ref %r bound %r' % (
        what, i, int(lab[i]), float(loss[i]), float(ref.loss[i]), float(ref.loss_bound[i]))
    i, j = divmod(int(rg.argmax()), k)
    assert float(rg.max()) <= 1.0, '%s: dlogits[%d, %d] %r ref %r bound %r' % (
        what, i, j, float(dz[i, j]), float(ref.dlogits[i, j]), float(ref.grad_bound[i, j]))
    assert float(rs.max()) <= 1.0, '%s: row %d: sum of dlogits %r' % (what, int(rs.argmax()), float(rsum[int(rs.argmax())]))
  print('K=%d: loss %.3g, gradient %.3g, row sum %.3g of the bound' % (k, worst[0], worst[1], worst[2]))


# ---------------------------------------------------------------------------------------------------------------------
# global average pooling
# ---------------------------------------------------------------------------------------------------------------------
def _offset_copy(t, pad=2):
  """A contiguous device copy of ``t`` that starts ``pad`` elements into a larger buffer: 4-byte, not 16-byte aligned."""
  buf = torch.empty(t.numel() + pad + 8, dtype=t.dtype, device=DEV)
  buf = buf[((-buf.data_ptr()) % 16) // 2:]                  # 16-byte aligned start, whatever the allocator gave
  v = buf[pad:pad + t.numel()].view(t.shape)
  v.copy_(t)
  assert v.is_contiguous() and v.data_ptr() % 16 == 2 * pad and v.data_ptr() % 4 == 0
  return v


@pytest.mark.parametrize('n', R.AVGPOOL_N)
def test_global_avgpool_matches_the_float64_reference(n):
  """Forward per element within 2^-8 |ref| + P * 2^-24 * mean_p |x| (the worst case of any fp32 summation order; a sum
  carried in bf16 misses it by orders of magnitude); both backward forms bit-identical to one fp32 division and one
  rounding.  For c % 8 == 0 the same through views that are 4-byte but not 16-byte aligned (the 2-channel kernels)."""
  from rigl_amd import _lib, ops
  worst = 0.0
  for (n_, p, c, kind) in R.avgpool_cases():
    if n_ != n:
      continue
    x = R.avgpool_input(n, p, c, kind)
    ref, mabs = R.avgpool_ref(x)
    bound = R.avgpool_fwd_bound(ref, mabs, p)
    xg = x.to(DEV).view(n, 1, p, c)
    forms = [('aligned', xg)]
    if c % 8 == 0:
      forms.append(('offset', _offset_copy(xg)))
    what = 'n=%d P=%d c=%d %s' % (n, p, c, kind)
    ys = []
    for form, xv in forms:
      y = ops.global_avgpool_fwd(xv).cpu()
      ratio = (y.double() - ref).abs() / bound.clamp(min=1e-300)
      worst = max(worst, float(ratio.max()))
      i, j = divmod(int(ratio.argmax()), c)
      assert float(ratio.max()) <= 1.0, '%s %s: y[%d, %d] %r ref %r bound %r' % (
          what, form, i, j, float(y[i, j]), float(ref[i, j]), float(bound[i, j]))
      ys.append(y)
    if len(ys) == 2:
      assert torch.equal(_bits(ys[0]), _bits(ys[1])), what + ': the 8- and 2-channel forms add in different orders'
    dy = R.avgpool_dy(n, c)
    dyg = dy.to(DEV)
    want = _bits(R.avgpool_bwd_ref(dy, p))
    assert torch.equal(_bits(ops.global_avgpool_bwd(dyg, 1, p)).view(n, p, c), want), what + ': backward'
    if c % 8 == 0:
      assert torch.equal(_bits(ops.global_avgpool_bwd(_offset_copy(dyg), 1, p)).view(n, p, c), want), what + ': backward, offset'
      xr = torch.relu(x.float()).to(torch.bfloat16)
      got = ops.global_avgpool_bwd_relu(dyg, xr.to(DEV).view(n, 1, p, c))
      assert torch.equal(_bits(got).view(n, p, c), _bits(R.avgpool_bwd_ref(dy, p, xr))), what + ': backward through relu'
      if p * c <= 4096:
        with pytest.raises(_lib.RiglError):                 # the ReLU form requires 16-byte alignment: an argument check
          ops.global_avgpool_bwd_relu(_offset_copy(dyg), xr.to(DEV).view(n, 1, p, c))
  print('n=%d: worst forward error / bound %.3g' % (n, worst))


# ---------------------------------------------------------------------------------------------------------------------
# batched entry points
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('count', [1, 63, 64, 65, 129, 200])
def test_pack_weights_batched_across_the_64_tensor_launches(count):
  """Every output, pre-filled with a sentinel, bit-identical to the NumPy reference and to the single-tensor call."""
  from rigl_amd import ops
  items = R.pack_items(count, count)
  layers, singles, refs = [], [], []
  for w, mask, want_hwio, want_ohwi in items:
    k, cout = w.shape
    tw = torch.from_numpy(w.reshape(-1)).to(DEV)
    bits = ops.mask_pack(torch.from_numpy(mask.reshape(-1)).to(DEV)) if mask is not None else None
    outs = [_sentinel_bf16((k * cout,)) if want else None for want in (want_hwio, want_ohwi) * 2]
    layers.append((tw, bits, k, cout, outs[0], outs[1]))
    singles.append((tw, bits, k, cout, outs[2], outs[3]))
    refs.append(R.pack_weights_ref(w, mask))
  ops.pack_weights_batched(layers)
  for s in singles:
    ops.pack_weights(*s)
  torch.cuda.synchronize()
  for i, (lay, sing, ref) in enumerate(zip(layers, singles, refs)):
    for nm, got, one, want in (('hwio', lay[4], sing[4], ref[0]), ('ohwi', lay[5], sing[5], ref[1])):
      if got is None:
        continue
      assert torch.equal(_bits(got), _bits(want).view(-1)), 'tensor %d of %d (k=%d cout=%d): %s' % (i, count, lay[2], lay[3], nm)
      assert torch.equal(_bits(one), _bits(want).view(-1)), 'tensor %d alone: %s' % (i, nm)


class _Var:
  def __init__(self, t):
    self.data = t


class _Bn:
  pass


@pytest.mark.parametrize('count', [1, 64, 65, 130])
def test_bn_infer_params_across_the_64_item_launches(count):
  """Bit-identical to the same items passed one per call; scale within 1e-6 |scale| and shift within
  1e-6 (|beta| + |mean * scale|) of the header's formula in float64 (`beta - mean * scale` may be contracted or not)."""
  from rigl_amd import ops
  items = R.bn_infer_items(count, count)
  bns = []
  for gamma, beta, mean, var, eps in items:
    b = _Bn()
    b.gamma, b.beta = _Var(torch.from_numpy(gamma).to(DEV)), _Var(torch.from_numpy(beta).to(DEV))
    b.moving_mean, b.moving_variance, b.eps = torch.from_numpy(mean).to(DEV), torch.from_numpy(var).to(DEV), eps
    bns.append(b)
  total = sum(2 * it[0].size for it in items)
  out = torch.full((total,), SENTINEL32, dtype=torch.int32, device=DEV).view(torch.float32)
  views = ops.bn_infer_params(bns, out=out)
  alone = [ops.bn_infer_params([b])[0] for b in bns]
  torch.cuda.synchronize()
  assert not (out.view(torch.int32) == SENTINEL32).any(), 'items never written'
  worst = 0.0
  for i, (it, v, a) in enumerate(zip(items, views, alone)):
    assert torch.equal(v.view(torch.int32), a.view(torch.int32)), 'item %d of %d (c=%d): not the bits of its own call' % (i, count, it[0].size)
    scale, shift, bs, bh = R.bn_infer_ref(*it)
    got = v.cpu().numpy().astype(np.float64)
    rs, rh = np.abs(got[0] - scale) / bs, np.abs(got[1] - shift) / np.maximum(bh, 1e-300)
    worst = max(worst, float(rs.max()), float(rh.max()))
    assert rs.max() <= 1.0 and rh.max() <= 1.0, 'item %d of %d (c=%d): scale %.3g, shift %.3g of the bound' % (
        i, count, it[0].size, rs.max(), rh.max())
  print('%d items: worst error / bound %.3g' % (count, worst))


@pytest.mark.parametrize('count', [1, 32, 33, 65])
def test_topk_mask_batched_across_the_32_layer_tables(count):
  """Bit-identical to oracle topk_order (ties: lower index first) and to ops.topk_mask layer by layer; the mask words start
  from the same sentinel in both calls."""
  from rigl_amd import ops
  items = R.topk_items(count, count)
  batch, alone = [], []
  for s, keep in items:
    ts = torch.from_numpy(s).to(DEV)
    words = ops.n_mask_words(s.size)
    batch.append((ts, keep, torch.full((words,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)))
    alone.append(ops.topk_mask(ts, keep, out=torch.full((words,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)))
  ops.topk_mask_batched(batch)
  torch.cuda.synchronize()
  for i, ((s, keep), (_, _, bits), one) in enumerate(zip(items, batch, alone)):
    what = 'layer %d of %d (n=%d keep=%d)' % (i, count, s.size, keep)
    got = ops.mask_unpack(bits, (s.size,)).cpu().numpy()
    assert np.array_equal(got, R.topk_ref(s, keep)), what + ': not the top-k of topk_order'
    assert torch.equal(bits, one), what + ': not the words of its own call'
