"""The references of tests/glue_ref.py checked without a GPU, and the bounds of tests/test_glue_edges_gpu.py shown to be
reachable.

* Each reference against an independent formulation: F.max_pool2d(return_indices=True) on -inf padded float64 input (the
  values always; the argmax on inputs WITHOUT ties, where the order cannot matter), a brute-force Python loop on tied
  inputs for the order, autograd for the pooling gradient, F.cross_entropy(label_smoothing) in float64 for in-range
  labels, hand-computed rows for K = 1, all-equal logits and out-of-range labels, an integer-arithmetic bf16 rounding
  for the average pool's gradient and the weight packer.
* For every tolerance of the GPU file that is not bit-exact, a NumPy fp32 restatement of the kernel's documented formula
  (the comments of head.hip / pool.hip / bn.hip: fp32 accumulation in the kernel's order, one bf16 rounding at the
  store) runs on the very inputs the GPU test uses and must stay inside HALF the bound.  Where a bound has a bf16-store
  term 2^-8 |ref|, that term is the store's half ulp at its worst (just above a power of two) and a correct kernel uses
  it up, so it is granted in full and the half is taken of everything else: |got - ref| <= 2^-8 |ref| + rest / 2.
"""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
import torch.nn.functional as F  # noqa: E402

from tests import convref, glue_ref as R  # noqa: E402

F32 = np.float32


def _bf16_bits_np(a):
  """Round-to-nearest-even fp32 -> bf16 bit patterns with integer arithmetic (finite inputs)."""
  u = np.ascontiguousarray(a, F32).view(np.uint32).astype(np.uint64)
  return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.int64)


def _bf16_np(a):
  return (_bf16_bits_np(a).astype(np.uint32) << 16).view(F32)


# ---------------------------------------------------------------------------------------------------------------------
# max pooling
# ---------------------------------------------------------------------------------------------------------------------
GEOMS = R.small_pool_geometries()


def _torch_pool(x64, d, want_idx=False):
  """F.max_pool2d on the -inf padded NCHW float64 image, cropped to the descriptor's output."""
  pb = max((d.ho - 1) * d.stride_h + d.kh - d.h - d.pad_top, 0)
  pr = max((d.wo - 1) * d.stride_w + d.kw - d.w - d.pad_left, 0)
  xp = F.pad(x64.permute(0, 3, 1, 2), (d.pad_left, pr, d.pad_top, pb), value=float('-inf'))
  y, idx = F.max_pool2d(xp, (d.kh, d.kw), (d.stride_h, d.stride_w), return_indices=True)
  y, idx = y[:, :, :d.ho, :d.wo], idx[:, :, :d.ho, :d.wo]
  if not want_idx:
    return y.permute(0, 2, 3, 1)
  wp = xp.shape[3]
  r = idx // wp - torch.arange(d.ho).view(1, 1, -1, 1) * d.stride_h
  s = idx % wp - torch.arange(d.wo).view(1, 1, 1, -1) * d.stride_w
  return y.permute(0, 2, 3, 1), (r * d.kw + s).permute(0, 2, 3, 1)


def _tie_free(d, seed):
  """Every (image, channel) plane a permutation of distinct small integers (exact in bf16)."""
  g = torch.Generator().manual_seed(seed)
  assert d.h * d.w <= 500
  perm = torch.rand(d.n, d.cin, d.h * d.w, generator=g).argsort(dim=-1).float() * 0.5 - 100.0
  return perm.view(d.n, d.cin, d.h, d.w).permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)


@pytest.mark.parametrize('name,d', GEOMS, ids=[g[0] for g in GEOMS])
def test_maxpool_ref_values_match_torch_on_every_input_kind(name, d):
  for i, kind in enumerate(R.POOL_INPUT_KINDS):
    x = R.pool_input(kind, d, 100 + i)
    y, arg = R.maxpool_ref(x, d)
    assert torch.equal(y.double(), _torch_pool(x.double(), d)), kind       # (+0 == -0 here: the bits are pinned below)
    assert int(arg.max()) < d.kh * d.kw
    if kind == 'infinities':
      assert (y.float() > float('-inf')).all() and (x.float() == float('-inf')).any() and (x.float() == float('inf')).any()
    if kind == 'negative':
      assert (y.float() < 0).all()


@pytest.mark.parametrize('name,d', GEOMS, ids=[g[0] for g in GEOMS])
def test_maxpool_ref_argmax_and_gradient_match_torch_without_ties(name, d):
  x = _tie_free(d, 5)
  y, arg = R.maxpool_ref(x, d)
  xr = x.double().requires_grad_(True)
  yr, ar = _torch_pool(xr, d, want_idx=True)
  assert torch.equal(y.double(), yr.detach())
  assert torch.equal(arg.to(torch.int64), ar)
  dy = R.pool_dy(d, 5)
  yr.backward(dy.double())
  dx, ab, cnt = R.maxpool_bwd_ref(dy, arg, d)
  assert torch.equal(dx, xr.grad)                         # sums of a few bf16 values are exact in float64
  assert (ab >= dx.abs()).all() and torch.equal(cnt == 0, ab == 0) or (dy.float() == 0).any()
  assert int(cnt.sum()) == dy.numel()                     # every window gives its gradient to exactly one pixel


@pytest.mark.parametrize('name,d', GEOMS, ids=[g[0] for g in GEOMS])
def test_maxpool_ref_tie_order_matches_a_brute_force_loop(name, d):
  """First maximum in row-major window order, the selected BITS (signed zeros) and clipped windows, element by element."""
  d = d._replace(n=1, cin=8)
  for kind in ('four_levels', 'signed_zeros', 'constant', 'infinities'):
    x = R.pool_input(kind, d, 3)
    y, arg = R.maxpool_ref(x, d)
    xf, xb, yb = x.float().numpy(), R.bits16(x).numpy(), R.bits16(y).numpy()
    for ho in range(d.ho):
      for wo in range(d.wo):
        for c in range(d.cin):
          best = None
          for r in range(d.kh):
            for s in range(d.kw):
              hi, wi = ho * d.stride_h - d.pad_top + r, wo * d.stride_w - d.pad_left + s
              if 0 <= hi < d.h and 0 <= wi < d.w and (best is None or xf[0, hi, wi, c] > best[0]):
                best = (xf[0, hi, wi, c], xb[0, hi, wi, c], r * d.kw + s)
          assert best is not None and (yb[0, ho, wo, c], int(arg[0, ho, wo, c])) == (best[1], best[2]), (kind, ho, wo, c)


def test_bn_relu_ref_is_one_fma_one_relu_one_rounding():
  d = GEOMS[0][1]
  x = R.pool_input('normal', d, 1)
  scale, shift = R.bn_relu_params(d.cin, 'zeros')
  got = R.bn_relu_ref(x, scale, shift)
  v = np.maximum(x.float().numpy().astype(np.float64) * scale.numpy().astype(np.float64) + shift.numpy().astype(np.float64), 0)
  assert np.array_equal(R.bits16(got).numpy(), _bf16_bits_np(v.astype(F32)))
  assert float((got == 0).float().mean()) > 0.5           # whole windows at +0
  ident = R.bn_relu_ref(x, *R.bn_relu_params(d.cin, 'identity'))
  assert torch.equal(ident, torch.relu(x.float()).to(torch.bfloat16))


def _maxpool_bwd_fp32(dy, arg, d):
  """pool.hip's backward: an fp32 accumulator per input element, the candidate windows added in (r, s) ascending order,
  one round-to-nearest-even store."""
  acc = np.zeros((d.n, d.h, d.w, d.cin), F32)
  dyf, a = dy.float().numpy(), arg.numpy()
  for r in range(d.kh):
    for s in range(d.kw):
      rg = R._tap_ranges(d, r, s)
      if rg is None:
        continue
      oh, ow, ih, iw = rg
      acc[:, ih, iw, :] += np.where(a[:, oh, ow, :] == r * d.kw + s, dyf[:, oh, ow, :], F32(0))
  return torch.from_numpy(_bf16_np(acc))


@pytest.mark.parametrize('name,d', GEOMS, ids=[g[0] for g in GEOMS])
def test_maxpool_bwd_bound_holds_for_the_fp32_restatement(name, d):
  for i, kind in enumerate(R.POOL_INPUT_KINDS):
    x = R.pool_input(kind, d, 100 + i)
    _, arg = R.maxpool_ref(x, d)
    dy = R.pool_dy(d, 100 + i)
    dx, ab, cnt = R.maxpool_bwd_ref(dy, arg, d)
    got = _maxpool_bwd_fp32(dy, arg, d)
    assert convref.check_close('%s %s dx' % (name, kind), got, dx, ab, rel=0.5e-5, out_ulp=2.0**-8) <= 1.0
    one = cnt <= 1
    assert torch.equal(R.bits16(got.to(torch.bfloat16))[one], R.bits16(dx.to(torch.bfloat16))[one])
    assert (got[cnt == 0] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# global average pooling
# ---------------------------------------------------------------------------------------------------------------------
def test_avgpool_refs_against_numpy():
  for (n, p, c, kind) in [(5, 49, 10, 'randn'), (1, 196, 8, '100+randn'), (5, 1, 6, 'randn')]:
    x = R.avgpool_input(n, p, c, kind)
    ref, mabs = R.avgpool_ref(x)
    xn = x.float().numpy().astype(np.longdouble)
    np.testing.assert_allclose(ref.numpy(), xn.mean(1).astype(np.float64), rtol=1e-14, atol=1e-15)
    np.testing.assert_allclose(mabs.numpy(), np.abs(xn).mean(1).astype(np.float64), rtol=1e-14)
    dy = R.avgpool_dy(n, c)
    q = _bf16_bits_np(dy.float().numpy() / F32(p))         # one IEEE fp32 division, then RNE
    got = R.bits16(R.avgpool_bwd_ref(dy, p)).numpy()
    assert got.shape == (n, p, c) and np.array_equal(got, np.broadcast_to(q[:, None, :], got.shape))
    xr = torch.relu(x.float()).to(torch.bfloat16)
    gated = R.bits16(R.avgpool_bwd_ref(dy, p, xr)).numpy()
    assert np.array_equal(gated, np.where(xr.float().numpy() > 0, got, 0))
  assert R.avgpool_input(2, 3, 8, 'randn', pad=2).storage_offset() == 2


def test_avgpool_cases_cover_the_grid():
  cases = R.avgpool_cases()
  assert {c[:3] for c in cases} == {(n, p, c) for n in R.AVGPOOL_N for p in R.AVGPOOL_P for c in R.AVGPOOL_C
                                    if n * p * c <= R.AVGPOOL_MAX_ELEMS}
  assert {c[3] for c in cases if c[0] * c[1] * c[2] >= R.AVGPOOL_BOTH_KINDS_BELOW} == {'randn', '100+randn'}
  for n in R.AVGPOOL_N:
    for p in R.AVGPOOL_P:
      assert any(c[0] == n and c[1] == p for c in cases)


@pytest.mark.parametrize('case', R.avgpool_cases(), ids=lambda c: '%dx%dx%d-%s' % c)
def test_avgpool_fwd_bound_holds_for_the_fp32_restatement(case):
  """head.hip: an fp32 accumulator per (image, channel), the pixels added in ascending order, one fp32 division by P, one
  bf16 rounding.  A sum carried in bf16 misses the bound by orders of magnitude (checked on the 196-pixel cases)."""
  n, p, c, kind = case
  x = R.avgpool_input(n, p, c, kind)
  ref, mabs = R.avgpool_ref(x)
  xf = x.float().numpy()
  acc = np.zeros((n, c), F32)
  for q in range(p):
    acc += xf[:, q, :]
  got = torch.from_numpy(_bf16_np(acc / F32(p))).double()
  ratio = float(((got - ref).abs() / R.avgpool_fwd_bound(ref, mabs, p, share=0.5)).max())
  assert ratio <= 1.0, ratio
  if p == 196 and n == 1:
    b = torch.zeros(n, c, dtype=torch.bfloat16)
    for q in range(p):
      b = (b.float() + x[:, q, :].float()).to(torch.bfloat16)
    bad = (((b.float() / p).double() - ref).abs() / R.avgpool_fwd_bound(ref, mabs, p)).max()
    assert float(bad) > 1.0


# ---------------------------------------------------------------------------------------------------------------------
# softmax cross-entropy
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [2, 10, 257, 1000])
@pytest.mark.parametrize('eps', R.XENT_EPS)
def test_xent_ref_matches_torch_float64_for_in_range_labels(k, eps):
  z, lab = R.xent_inputs(128, k, 0)
  inr = (lab >= 0) & (lab < k)
  assert inr.any() and not inr.all()
  zr = z[inr].double().requires_grad_(True)
  rows = F.cross_entropy(zr, lab[inr], label_smoothing=float(np.float32(eps)), reduction='none')
  (rows.sum() * 0.25).backward()
  ref = R.xent_ref(z, lab, eps, 0.25)
  assert torch.allclose(ref.loss[inr], rows.detach(), rtol=1e-12, atol=1e-12)
  assert torch.allclose(ref.dlogits[inr], zr.grad, rtol=1e-12, atol=1e-15)
  assert torch.allclose(ref.p.sum(1), torch.ones(128, dtype=torch.float64), rtol=1e-12)


def test_xent_ref_hand_computed_rows():
  bf = lambda a: torch.tensor(a, dtype=torch.float32).to(torch.bfloat16)     # noqa: E731
  # K = 1: p = 1, log p = 0: the loss is 0 for every label; in range t = 1, out of range t = eps
  r = R.xent_ref(bf([[3.5], [3.5], [-7.0]]), torch.tensor([0, 1, -1]), 0.25, 2.0)
  assert r.loss.tolist() == [0.0, 0.0, 0.0]
  assert r.dlogits[:, 0].tolist() == [0.0, 1.5, 1.5] and r.t[:, 0].tolist() == [1.0, 0.25, 0.25]
  # all-equal logits: p = 1 / K, loss = log K whatever eps; out of range only the smoothing term is left: eps * log K
  k = 8
  z = bf([[2.0] * k] * 3)
  r = R.xent_ref(z, torch.tensor([5, k, -1]), 0.5, 1.0)
  np.testing.assert_allclose(r.loss.numpy(), [np.log(k), 0.5 * np.log(k), 0.5 * np.log(k)], rtol=1e-15)
  np.testing.assert_allclose(r.dlogits[1].numpy(), np.full(k, 1.0 / k - 0.5 / k), rtol=1e-15)
  np.testing.assert_allclose(r.dlogits[0].numpy(), np.where(np.arange(k) == 5, 1.0 / k - 0.5 - 0.5 / k, 0.5 / k), rtol=1e-14)
  # tf.one_hot: an out-of-range label with eps = 0 has no target at all: loss 0, dlogits = p
  r = R.xent_ref(bf([[0.0, 1.0, 2.0]]), torch.tensor([3]), 0.0, 1.0)
  assert float(r.loss[0]) == 0.0 and torch.equal(r.dlogits, r.p) and float(r.t.abs().max()) == 0.0
  # two classes, label 0, no smoothing: loss = log(1 + e^(z1 - z0))
  r = R.xent_ref(bf([[1.0, 3.0]]), torch.tensor([0]), 0.0, 1.0)
  np.testing.assert_allclose(float(r.loss[0]), np.log1p(np.exp(2.0)), rtol=1e-15)


def test_xent_inputs_hold_every_pair_of_kinds():
  z, lab = R.xent_inputs(128, 1000, 0)
  zf = z.float()
  assert (lab == -1).sum() >= 12 and (lab == 1000).sum() >= 12 and (lab == 0).sum() >= 12 and (lab == 999).sum() >= 12
  assert float(zf[1].min()) > 100 and float(zf[2].max()) < -100             # exp of the raw logits: inf / 0 in fp32
  with np.errstate(over='ignore'):
    assert np.isinf(np.exp(zf[1].numpy())).all() and (np.exp(zf[2].numpy()) == 0).all()
  assert float(zf[4].max()) == float(zf[4].min()) and int((zf[5] == zf[5].max()).sum()) == 2
  r = R.xent_ref(z, lab, 0.0, 1.0)
  assert float(r.loss[3]) < 0.02 and lab[3] >= 0                             # the dominant logit sits on the label


def _strided_sum(a):
  """The block's reduction order of head.hip: thread t adds elements t, t + 256, ... in order; then the 256 partials."""
  rows, k = a.shape
  pad = (-k) % 256
  a = np.concatenate([a, np.zeros((rows, pad), F32)], axis=1).reshape(rows, -1, 256)
  part = np.zeros((rows, 256), F32)
  for i in range(a.shape[1]):
    part += a[:, i, :]
  while part.shape[1] > 1:                                  # butterfly
    part = part[:, 0::2] + part[:, 1::2]
  return part[:, 0]


def _xent_fp32(z_bf16, labels, eps, grad_scale):
  """head.hip's formula in NumPy fp32: m = max, v = z - m, se = sum exp(v), sz = sum v, lse = log se,
  loss = on * (lse - v_lab) [label in range] + off * (K * lse - sz), dlogits = bf16((exp(v - lse) - t) * scale)."""
  z = z_bf16.float().numpy()
  rows, k = z.shape
  lab = labels.numpy()
  v = (z - z.max(1, keepdims=True)).astype(F32)
  se, sz = _strided_sum(np.exp(v)), _strided_sum(v)
  lse = np.log(se).astype(F32)
  on, off = F32(1) - F32(eps), F32(eps) / F32(k)
  inr = (lab >= 0) & (lab < k)
  vl = np.where(inr, v[np.arange(rows), np.clip(lab, 0, k - 1)], F32(0)).astype(F32)
  smooth = (off * (F32(k) * lse - sz).astype(F32)).astype(F32)
  loss = np.where(inr, (on * (lse - vl).astype(F32)).astype(F32) + smooth, smooth).astype(F32)
  p = np.exp((v - lse[:, None]).astype(F32)).astype(F32)
  t = np.full((rows, k), off, F32)
  t[np.arange(rows)[inr], lab[inr]] += on
  g = ((p - t).astype(F32) * F32(grad_scale)).astype(F32)
  return loss, torch.from_numpy(_bf16_np(g))


def _xent_ratios(rows, k, seed, eps, gs, spread=R.XENT_SPREAD):
  z, lab = R.xent_inputs(rows, k, seed, spread=spread)
  ref = R.xent_ref(z, lab, eps, gs)
  loss, g = _xent_fp32(z, lab, eps, gs)
  rl = float(((torch.from_numpy(loss).double() - ref.loss).abs() / ref.loss_bound).max())
  half = ref.grad_store + 0.5 * (ref.grad_bound - ref.grad_store)
  rg = 0.5 * float(((g.double() - ref.dlogits).abs() / half).max())        # 0.5 = the whole of the halved bound
  inr = (lab >= 0) & (lab < k)
  strict = R.xent_row_sum_rows(ref, lab, gs)
  rsum = g.double().sum(1).abs()
  rs = float((rsum / R.xent_row_sum_bound(g, k).clamp(min=1e-300))[strict].max()) if strict.any() else 0.0
  loose = inr & ~strict
  if loose.any():
    rs = max(rs, float((rsum / R.xent_row_sum_fp32_bound(ref, g).clamp(min=1e-300))[loose].max()))
  return rl, rg, rs


@pytest.mark.parametrize('k', R.XENT_K)
def test_xent_bounds_hold_for_the_fp32_restatement(k):
  """Loss, gradient and row-sum bounds on the inputs of the GPU sweep: the fp32 restatement needs at most half of the loss
  bound and of the gradient bound's fp32 part.  The row-sum bound is made of bf16-store half ulps alone and is reached
  exactly when K = 2 entries of one magnitude round in opposite directions: it is required in full."""
  worst = [0.0, 0.0, 0.0]
  for rows, seed, eps, gs in R.xent_sweep(k):
    worst = [max(a, b) for a, b in zip(worst, _xent_ratios(rows, k, seed, eps, gs))]
  print('K=%d: loss %.3g, gradient %.3g, row sum %.3g of the bound' % (k, *worst))
  assert max(worst[:2]) <= 0.5 and worst[2] <= 1.0, worst


def test_xent_spread_is_the_largest_power_of_two():
  """At twice XENT_SPREAD the offset rows reach z - m below -104, where exp is zero in fp32 and the reference is not: the
  restatement misses the gradient bound (got 0, error = |ref| > 2^-8 |ref| + 1e-5 |scale| p |z - m - lse|)."""
  _, rg, _ = _xent_ratios(128, 20000, 0, 0.0, 1.0, spread=2 * R.XENT_SPREAD)
  assert rg > 1.0, rg
  _, rg, _ = _xent_ratios(128, 20000, 0, 0.0, 1.0)
  assert rg <= 0.5, rg


# ---------------------------------------------------------------------------------------------------------------------
# batched helpers
# ---------------------------------------------------------------------------------------------------------------------
def test_pack_weights_ref_is_round_to_nearest_even_of_the_masked_weights():
  for w, mask, _, _ in R.pack_items(12, 1):
    hwio, ohwi = R.pack_weights_ref(w, mask)
    want = _bf16_bits_np(w if mask is None else np.where(mask != 0, w, F32(0)))
    assert np.array_equal(R.bits16(hwio).numpy(), want) and np.array_equal(R.bits16(ohwi).numpy(), want.T)
  items = R.pack_items(200, 0)
  for b in (64, 128):
    near = items[b - 3:b + 3]
    assert any(m is None for _, m, _, _ in near[:3]) and any(m is not None for _, m, _, _ in near[:3])
    assert any(m is None for _, m, _, _ in near[3:]) and any(m is not None for _, m, _, _ in near[3:])
  assert any(not h for _, _, h, _ in items) and any(not o for _, _, _, o in items)
  assert any(w.shape[0] % 8 and w.shape[1] % 8 for w, _, _, _ in items)


def test_bn_infer_bound_holds_for_the_fp32_restatement():
  """bn.hip: invstd = float(1 / sqrt(double(var) + eps)), scale = gamma * invstd, shift = beta - mean * scale in fp32,
  with and without the product contracted into an fma."""
  worst = 0.0
  for gamma, beta, mean, var, eps in R.bn_infer_items(130, 0):
    scale, shift, bs, bh = R.bn_infer_ref(gamma, beta, mean, var, eps)
    invstd = (1.0 / np.sqrt(var.astype(np.float64) + np.float64(F32(eps)))).astype(F32)
    sc = (gamma * invstd).astype(F32)
    plain = (beta - (mean * sc).astype(F32)).astype(F32)
    fused = (beta.astype(np.float64) - mean.astype(np.float64) * sc.astype(np.float64)).astype(F32)
    worst = max(worst, float((np.abs(sc - scale) / bs).max()), float((np.abs(plain - shift) / np.maximum(bh, 1e-300)).max()),
                float((np.abs(fused - shift) / np.maximum(bh, 1e-300)).max()))
  assert worst <= 0.5, worst
  assert any(g.size > 256 for g, *_ in R.bn_infer_items(130, 0))


def test_topk_items_and_ref():
  items = R.topk_items(65, 0)
  assert sum(s.size == 300007 for s, _ in items) == 1 and all(s.size % 32 for s, _ in items)
  assert any(k == 0 for _, k in items) and any(k == s.size for s, k in items)
  s, k = np.array([1, 3, 3, 0, 3, 2], F32), 3
  assert R.topk_ref(s, k).tolist() == [0, 1, 1, 0, 1, 0] and R.topk_ref(s, 2).tolist() == [0, 1, 1, 0, 0, 0]
  tied = 0
  for s, k in items:
    if 0 < k < s.size:
      ref = R.topk_ref(s, k)
      thr = s[ref == 1].min()
      tied += bool((s[ref == 0] == thr).any())              # a score equal to the threshold is left out: a tie across it
  assert tied >= 5
