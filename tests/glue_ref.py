"""Plain high-precision references for the glue kernels -- TEST INFRASTRUCTURE, never imported by the product.

Max pooling, global average pooling, softmax cross-entropy and the batched helpers (weight packing, frozen batch-norm
parameters) restated with torch CPU tensors in float64 / NumPy: a Python loop over the kh * kw window taps, vectorised
over everything else.  Nothing here touches a GPU or the library, so tests/test_glue_ref_cpu.py can check every
reference against an independent formulation; tests/test_glue_edges_gpu.py then holds the HIP kernels to them.

The input generators and the tolerance formulas live here as well: the CPU file runs a NumPy fp32 restatement of each
kernel's documented formula on the very inputs the GPU file uses and requires it to stay inside HALF of each bound,
which is how the bounds are shown to be reachable before a GPU is involved.
"""
import collections

import numpy as np
import torch

# The fields of RiglConvDesc a pooling reads (ops.conv_desc builds the ctypes twin; cin == cout).
PoolDesc = collections.namedtuple('PoolDesc', 'n h w cin ho wo kh kw stride_h stride_w pad_top pad_left')


def pool_desc(n, h, w, c, kh, kw, stride, pad_top, pad_left, ho, wo):
  sh, sw = (stride, stride) if isinstance(stride, int) else stride
  return PoolDesc(n, h, w, c, ho, wo, kh, kw, sh, sw, pad_top, pad_left)


def same_pool_desc(n, h, w, c, k, s):
  """TF 'SAME': ho = ceil(h / s), the padding split with the smaller half in front."""
  ho, wo = -(-h // s), -(-w // s)
  ph, pw = max((ho - 1) * s + k - h, 0), max((wo - 1) * s + k - w, 0)
  return pool_desc(n, h, w, c, k, k, s, ph // 2, pw // 2, ho, wo)


def valid_pool_desc(n, h, w, c, k, s):
  return pool_desc(n, h, w, c, k, k, s, 0, 0, (h - k) // s + 1, (w - k) // s + 1)


def bits16(t):
  """bf16 tensor -> its bit patterns as an int32 tensor in [0, 65535]."""
  return t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def from_bits16(b):
  """int tensor of bit patterns -> bf16 tensor."""
  b = b.to(torch.int32)
  return torch.where(b >= 32768, b - 65536, b).to(torch.int16).view(torch.bfloat16)


def _tap_ranges(d, r, s):
  """Output rows / columns whose tap (r, s) lies inside the image, and the input rows / columns they read."""
  def one(size, out, stride, pad, t):
    lo = max(0, -((t - pad) // stride))                       # ceil((pad - t) / stride)
    hi = min(out - 1, (size - 1 + pad - t) // stride)
    if hi < lo:
      return None
    return slice(lo, hi + 1), slice(lo * stride - pad + t, hi * stride - pad + t + 1, stride)
  a = one(d.h, d.ho, d.stride_h, d.pad_top, r)
  b = one(d.w, d.wo, d.stride_w, d.pad_left, s)
  return None if a is None or b is None else (a[0], b[0], a[1], b[1])


# ---------------------------------------------------------------------------------------------------------------------
# max pooling
# ---------------------------------------------------------------------------------------------------------------------
def maxpool_ref(x_bf16, d):
  """x [n, h, w, c] bf16 (CPU) -> (y bf16: the bit patterns of the winners, argmax uint8 = r * kw + s of the winner).
  Start from "no winner", visit the in-image taps in (r, s) ascending order, replace on strictly greater: the FIRST
  maximum in row-major window order.  Taps outside the image do not take part (they are not zeros).  A window without
  any in-image tap keeps argmax 0 and the bits of -inf (the library rejects such a descriptor)."""
  assert tuple(x_bf16.shape) == (d.n, d.h, d.w, d.cin) and x_bf16.dtype == torch.bfloat16
  xd = x_bf16.double()
  xb = x_bf16.contiguous().view(torch.int16)
  shape = (d.n, d.ho, d.wo, d.cin)
  best = torch.zeros(shape, dtype=torch.float64)
  has = torch.zeros(shape, dtype=torch.bool)
  yb = torch.full(shape, -128, dtype=torch.int16)             # 0xFF80 = -inf
  arg = torch.zeros(shape, dtype=torch.uint8)
  for r in range(d.kh):
    for s in range(d.kw):
      rg = _tap_ranges(d, r, s)
      if rg is None:
        continue
      oh, ow, ih, iw = rg
      v = xd[:, ih, iw, :]
      take = ~has[:, oh, ow, :] | (v > best[:, oh, ow, :])
      best[:, oh, ow, :] = torch.where(take, v, best[:, oh, ow, :])
      yb[:, oh, ow, :] = torch.where(take, xb[:, ih, iw, :], yb[:, oh, ow, :])
      arg[:, oh, ow, :] = torch.where(take, torch.tensor(r * d.kw + s, dtype=torch.uint8), arg[:, oh, ow, :])
      has[:, oh, ow, :] |= take
  return yb.view(torch.bfloat16), arg


def maxpool_bwd_ref(dy_bf16, argmax, d):
  """-> (dx float64 [n, h, w, c], sum of |terms| float64, number of terms int16): every window adds its dy to the
  input position its argmax names."""
  shape = (d.n, d.h, d.w, d.cin)
  dyd = dy_bf16.double()
  dx = torch.zeros(shape, dtype=torch.float64)
  ab = torch.zeros(shape, dtype=torch.float64)
  cnt = torch.zeros(shape, dtype=torch.int16)
  for r in range(d.kh):
    for s in range(d.kw):
      rg = _tap_ranges(d, r, s)
      if rg is None:
        continue
      oh, ow, ih, iw = rg
      sel = argmax[:, oh, ow, :] == (r * d.kw + s)
      term = torch.where(sel, dyd[:, oh, ow, :], torch.zeros((), dtype=torch.float64))
      dx[:, ih, iw, :] += term
      ab[:, ih, iw, :] += term.abs()
      cnt[:, ih, iw, :] += sel.to(torch.int16)
  return dx, ab, cnt


def bn_relu_ref(x_bf16, scale, shift):
  """bf16(relu(fma(x, scale, shift))) per channel, scale / shift fp32 [c]: the product of a bf16 and an fp32 value and
  its sum with an fp32 value of comparable size are exact in float64, so one rounding to fp32 is the fma."""
  v = (x_bf16.double() * scale.double() + shift.double()).float()
  return torch.where(v > 0, v, torch.zeros((), dtype=torch.float32)).to(torch.bfloat16)


POOL_INPUT_KINDS = ('normal', 'four_levels', 'negative', 'constant', 'signed_zeros', 'infinities')


def pool_input(kind, d, seed):
  """The input images of the max-pool sweep, bf16 [n, h, w, c] on the CPU."""
  g = torch.Generator().manual_seed(seed)
  shape = (d.n, d.h, d.w, d.cin)
  x = torch.randn(shape, generator=g)
  if kind == 'normal':
    pass
  elif kind == 'four_levels':                                  # long ties inside every window
    x = torch.floor(x.clamp(-1.9, 1.9)) * 0.5
  elif kind == 'negative':                                     # a zero-padding bug wins every border window
    x = -x.abs() - 0.125
  elif kind == 'constant':
    x = torch.full(shape, -1.5)
  elif kind == 'signed_zeros':
    x = torch.where(x > 0, torch.tensor(0.0), torch.tensor(-0.0))
  elif kind == 'infinities':
    u = torch.rand(shape, generator=g)
    x = torch.where(u < 0.15, torch.tensor(float('-inf')), x)
    x = torch.where(u > 0.95, torch.tensor(float('inf')), x)
    # every window keeps a value above -inf: where a window holds nothing else, its first in-image tap becomes finite
    y, _ = maxpool_ref(x.to(torch.bfloat16), d)
    n_i, ho_i, wo_i, c_i = (y.float() == float('-inf')).nonzero(as_tuple=True)
    hi = (ho_i * d.stride_h - d.pad_top).clamp(min=0)
    wi = (wo_i * d.stride_w - d.pad_left).clamp(min=0)
    x[n_i, hi, wi, c_i] = 0.5
  else:
    raise ValueError(kind)
  return x.to(torch.bfloat16)


def pool_dy(d, seed):
  g = torch.Generator().manual_seed(seed + 7919)
  return torch.randn((d.n, d.ho, d.wo, d.cin), generator=g).to(torch.bfloat16)


def small_pool_geometries():
  """(name, PoolDesc) of the sweep; channels 8, 24 and 64 in rotation."""
  return [
      ('3x3s2_same_even', same_pool_desc(2, 16, 16, 64, 3, 2)),            # pad_top 0
      ('3x3s2_same_odd', same_pool_desc(3, 15, 13, 8, 3, 2)),              # pad_top 1
      ('3x3s2_valid_one_trailing', valid_pool_desc(2, 16, 14, 24, 3, 2)),  # row 15 / column 13 behind the last window
      ('3x3s2_valid_two_trailing', pool_desc(2, 17, 19, 8, 3, 3, 2, 0, 0, 7, 8)),   # rows 15, 16 / columns 17, 18
      ('3x3s2_valid_odd', valid_pool_desc(1, 15, 9, 24, 3, 2)),            # no trailing row
      ('3x3s2_pad2', pool_desc(2, 14, 12, 64, 3, 3, 2, 2, 2, 8, 6)),       # first window: one in-image tap
      ('2x2s2_even', valid_pool_desc(2, 16, 12, 24, 2, 2)),
      ('2x2s2_odd', valid_pool_desc(2, 15, 13, 64, 2, 2)),                 # last row / column in no window
      ('3x3s1_same', same_pool_desc(2, 9, 10, 8, 3, 1)),
      ('2x3_s2x1', pool_desc(2, 9, 11, 24, 2, 3, (2, 1), 0, 1, 4, 11)),
      ('5x5s3_pad2', pool_desc(2, 17, 14, 8, 5, 5, 3, 2, 2, 6, 5)),
      ('window_larger_than_image', pool_desc(3, 3, 2, 64, 5, 5, 1, 2, 2, 3, 2)),
  ]


def bn_relu_params(c, which):
  """fp32 scale / shift [c] for the fused stem tail: 'identity' = (1, 0); 'zeros' sends most of a standard-normal image
  below zero, so whole windows tie at +0, and mixes in negative and fractional scales."""
  if which == 'identity':
    return torch.ones(c), torch.zeros(c)
  i = torch.arange(c)
  scale = torch.tensor([0.75, 1.0, -0.5, 1.25])[i % 4]
  shift = torch.tensor([-2.0, -3.0, -1.5, 0.25, -2.5])[i % 5]
  return scale.float(), shift.float()


# ---------------------------------------------------------------------------------------------------------------------
# global average pooling
# ---------------------------------------------------------------------------------------------------------------------
def avgpool_ref(x_bf16):
  """x [n, P, c] bf16 -> (mean over P in float64 [n, c], mean over P of |x|)."""
  xd = x_bf16.double()
  return xd.mean(dim=1), xd.abs().mean(dim=1)


def avgpool_bwd_ref(dy_bf16, pixels, x_bf16=None):
  """Bit-exact: one IEEE fp32 division float32(dy) / float32(P), round-to-nearest-even to bf16, the same value at every
  pixel; with x (the pooled ReLU output) the ReLU-gated form: times [x > 0] (+0 elsewhere)."""
  q = (dy_bf16.float() / torch.tensor(float(pixels), dtype=torch.float32)).to(torch.bfloat16)
  dx = q[:, None, :].expand(q.shape[0], pixels, q.shape[1])
  if x_bf16 is not None:
    dx = torch.where(x_bf16.float() > 0, dx, torch.zeros((), dtype=torch.bfloat16))
  return dx.contiguous()


def avgpool_fwd_bound(ref, mean_abs, pixels, share=1.0):
  """2^-8 |ref| (the bf16 store: half an ulp at worst, nothing to spare) + share * P * 2^-24 * mean_p |x| (the worst
  case of any fp32 summation order)."""
  return 2.0**-8 * ref.abs() + share * pixels * 2.0**-24 * mean_abs


AVGPOOL_P = (1, 49, 64, 196, 3136)
AVGPOOL_C = (2, 6, 8, 10, 1024, 2048)
AVGPOOL_N = (1, 5, 128)
AVGPOOL_MAX_ELEMS = 10**8
AVGPOOL_BOTH_KINDS_BELOW = 1 << 23


def avgpool_cases():
  """(n, P, c, kind): every (n, P, c) of at most about 1e8 elements; both input kinds ('randn', '100+randn') on the small
  ones, the two alternating on the large ones (the sweep is thinned there to bound the suite's wall time)."""
  out, flip = [], 0
  for n in AVGPOOL_N:
    for p in AVGPOOL_P:
      for c in AVGPOOL_C:
        if n * p * c > AVGPOOL_MAX_ELEMS:
          continue
        if n * p * c < AVGPOOL_BOTH_KINDS_BELOW:
          out += [(n, p, c, 'randn'), (n, p, c, '100+randn')]
        else:
          out.append((n, p, c, ('randn', '100+randn')[flip & 1]))
          flip += 1
  return out


def avgpool_input(n, p, c, kind, pad=0):
  """bf16 [n, P, c]; with pad > 0 a contiguous view that starts ``pad`` elements into a larger buffer."""
  g = torch.Generator().manual_seed(n * 1000003 + p * 1009 + c)
  buf = torch.randn(n * p * c + pad, generator=g)
  if kind == '100+randn':
    buf += 100.0
  return buf.to(torch.bfloat16)[pad:].view(n, p, c)


def avgpool_dy(n, c):
  g = torch.Generator().manual_seed(n * 31 + c)
  return torch.randn(n, c, generator=g).to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------------------
# softmax cross-entropy
# ---------------------------------------------------------------------------------------------------------------------
XentRef = collections.namedtuple('XentRef', 'loss dlogits p t m lse loss_bound grad_bound grad_store')


def xent_ref(z_bf16, labels, eps, grad_scale):
  """Row loss -sum_k t_k log softmax(z)_k and dlogits = (p - t) * grad_scale in float64 through a float64 log-sum-exp.
  Targets follow tf.one_hot: t = onehot * (1 - eps) + eps / K, and a label outside [0, K) has an all-zero one-hot row,
  so t = eps / K everywhere and the loss is the smoothing term alone.  eps is the fp32 value the library receives.
  Also returned: the two bounds of the GPU test, in the project's "1e-5 of the magnitudes of the terms" form
    loss : 1e-5 * (on * (lse + |z_lab - m|) + off * (K * lse + sum_k |z_k - m|)) + 1e-6   (no `on` term out of range)
    grad : 2^-8 |ref| + 1e-5 * |grad_scale| * (p * max(1, |z - m - lse|) + t)
  (grad_store is the first term alone: the bf16 store's half ulp, which a correct kernel may use up entirely)."""
  z = z_bf16.double()
  rows, k = z.shape
  e = float(np.float32(eps))
  on, off = 1.0 - e, e / k
  m = z.max(dim=1, keepdim=True).values
  s = z - m
  lse = torch.log(torch.exp(s).sum(dim=1, keepdim=True))
  logp = s - lse
  p = torch.exp(logp)
  lab = labels.to(torch.int64)
  inr = (lab >= 0) & (lab < k)
  t = torch.full((rows, k), off, dtype=torch.float64)
  ri = torch.arange(rows)[inr]
  t[ri, lab[inr]] += on
  loss = -(t * logp).sum(dim=1)
  dlogits = (p - t) * grad_scale
  s_lab = torch.zeros(rows, dtype=torch.float64)
  s_lab[ri] = s[ri, lab[inr]]
  lse1 = lse[:, 0]
  loss_bound = 1e-5 * (on * inr.double() * (lse1 + s_lab.abs()) + off * (k * lse1 + s.abs().sum(dim=1))) + 1e-6
  grad_store = 2.0**-8 * dlogits.abs()
  grad_bound = grad_store + 1e-5 * abs(grad_scale) * (p * logp.abs().clamp(min=1.0) + t)
  return XentRef(loss, dlogits, p, t, m[:, 0], lse1, loss_bound, grad_bound, grad_store)


XENT_K = (1, 2, 10, 37, 255, 256, 257, 1000, 1001, 5000, 8192, 20000)
XENT_EVAL_MAX_K = 8192              # rigl_eval_metrics stages the row in LDS
XENT_ROWS = (1, 128, 1024)
XENT_EPS = (0.0, 0.1, 1.0)
XENT_LOGIT_KINDS = ('randn3', 'plus200', 'minus200', 'dominant', 'all_equal', 'two_maxima')
XENT_LABEL_KINDS = ('random', 'zero', 'last', 'minus_one', 'k')
# The spread of the two offset kinds.  randn * 40 +- 200 was the first proposal; there z - m reaches -340 and below, and fp32
# cannot hold the softmax: exp(-104) is already zero in fp32 (the smallest denormal is 1.4e-45 = exp(-103.3)) while the
# float64 reference keeps p = 1e-148, so the fp32 restatement of head.hip's formula misses the gradient bound
# 2^-8 |ref| + 1e-5 |scale| p |z - m - lse| there (got 0, error = |ref|), at any spread of 16 or more for 20 000 classes
# (tests/test_glue_ref_cpu.py::test_xent_spread_is_the_largest_power_of_two).  8 is the largest power of two at which
# the restatement keeps half of both bounds; the offsets of +-200 stay, so an exp of the unshifted logits still
# overflows / flushes to zero.
XENT_SPREAD = 8.0


def xent_grad_scales(rows):
  return (1.0, 1.0 / rows, 128.0)


def xent_sweep(k):
  """(rows, seed, eps, grad_scale) of the sweep for K = k: every eps x grad_scale at every row count, except that 1024
  rows of more than 1001 classes run once (eps 0.1, scale 1 / rows: the float64 reference of 1024 x 20 000 logits costs
  a second per call); a single row rotates through the six logit kinds by seed."""
  out = []
  for rows in XENT_ROWS:
    if rows == 1024 and k > 1001:
      combos = [(XENT_EPS[1], 1.0 / rows)]
    else:
      combos = [(e, gs) for e in XENT_EPS for gs in xent_grad_scales(rows)]
    for seed in (range(6) if rows == 1 else (0,)):
      out += [(rows, seed, e, gs) for e, gs in combos]
  return out


def xent_inputs(rows, k, seed, spread=XENT_SPREAD):
  """(logits bf16 [rows, k], labels int64 [rows]): row i takes logit kind i % 6 and label kind (i // 6) % 5, so 30 rows
  hold every pair; with fewer rows the seed rotates the starting pair."""
  g = torch.Generator().manual_seed(seed * 7 + rows * 13 + k)
  z = torch.randn(rows, k, generator=g)
  lab = torch.randint(0, k, (rows,), generator=g)
  pos = torch.randint(0, k, (rows,), generator=g)
  pos2 = torch.randint(0, k, (rows,), generator=g)
  out = torch.empty(rows, k)
  for i in range(rows):
    j = i + seed
    lk = XENT_LABEL_KINDS[(j // 6) % 5]
    if lk == 'zero':
      lab[i] = 0
    elif lk == 'last':
      lab[i] = k - 1
    elif lk == 'minus_one':
      lab[i] = -1
    elif lk == 'k':
      lab[i] = k
    zk = XENT_LOGIT_KINDS[j % 6]
    if zk == 'randn3':
      out[i] = z[i] * 3.0
    elif zk == 'plus200':                                      # an exp of the unshifted logits overflows
      out[i] = z[i] * spread + 200.0
    elif zk == 'minus200':                                     # ... flushes to zero
      out[i] = z[i] * spread - 200.0
    elif zk == 'dominant':
      # one logit above the rest by 6 + ln K (on the label where it is in range): loss -> e^-6, and 1 - p_label stays
      # far above the fp32 rounding of p_label, which the row-sum assertion does not budget for
      out[i] = z[i] * 0.5
      at = int(lab[i]) if 0 <= int(lab[i]) < k else int(pos[i])
      out[i, at] = 6.0 + float(np.log(k))
    elif zk == 'all_equal':                                    # loss = log K
      out[i] = float(z[i, 0])
    else:                                                      # two equal maxima
      out[i] = z[i] * 3.0
      out[i, int(pos[i])] = 16.0
      out[i, int(pos2[i])] = 16.0
  return out.to(torch.bfloat16), lab


def xent_row_sum_bound(dlogits_bf16, k):
  """K bf16 half-ulps of the row's largest stored entry: what the stores alone may add to a row sum that is zero in exact
  arithmetic (sum_k p_k = sum_k t_k = 1 for a label in range)."""
  _, e = torch.frexp(dlogits_bf16.double().abs().max(dim=1).values)       # max = f * 2^e, f in [0.5, 1): ulp = 2^(e - 8)
  return k * torch.ldexp(torch.ones((), dtype=torch.float64), e - 9)


def xent_row_sum_rows(ref, labels, grad_scale):
  """The rows xent_row_sum_bound applies to: label in range and a largest entry of at least 2^-12 |grad_scale|.  The bound
  budgets for the bf16 stores only.  p and t are fp32 values of up to 1, so every entry (p - t) * scale carries an fp32
  error of about 2^-24 |scale| whatever its own size; in a row whose entries are all smaller than that by less than the
  2^9 between a bf16 half ulp and 1 -- all-equal logits with eps = 1, where the exact gradient is 0 and the stored one is
  K copies of one rounding error; two classes with a saturated softmax -- that error IS the row sum and no fp32 kernel
  can meet the bound.  Below 2^-12 |scale| (a half ulp of 2^-21 |scale|, 8 fp32 ulps of 1) the rows get the sum of
  their per-element fp32 allowances instead (xent_row_sum_fp32_bound)."""
  k = ref.p.shape[1]
  inr = (labels >= 0) & (labels < k)
  return inr & (ref.dlogits.abs().max(dim=1).values >= 2.0**-12 * abs(grad_scale))


def xent_row_sum_fp32_bound(ref, dlogits_bf16):
  """xent_row_sum_bound plus the row's sum of the gradient bound's fp32 parts: for in-range rows outside
  xent_row_sum_rows."""
  return xent_row_sum_bound(dlogits_bf16, ref.p.shape[1]) + (ref.grad_bound - ref.grad_store).sum(dim=1)


# ---------------------------------------------------------------------------------------------------------------------
# batched entry points
# ---------------------------------------------------------------------------------------------------------------------
def pack_weights_ref(w, mask=None):
  """w fp32 [k, cout] (NumPy), mask 0/1 of the same shape or None -> bf16 tensors (hwio [k, cout], ohwi [cout, k]):
  hwio = bf16(mask ? w : +0), round to nearest even; ohwi its transpose."""
  w = np.asarray(w, np.float32)
  if mask is not None:
    w = np.where(np.asarray(mask) != 0, w, np.float32(0))
  hwio = torch.from_numpy(np.ascontiguousarray(w)).to(torch.bfloat16)
  return hwio, hwio.t().contiguous()


PACK_SHAPES = ((64, 64), (147, 64), (7, 10), (100, 12), (1, 8), (128, 1000), (12, 7), (576, 64), (65, 129), (256, 4))


def pack_items(count, seed):
  """``count`` tensors of mixed (k, cout) as NumPy (w [k, cout], mask or None, want_hwio, want_ohwi).  Masked and
  unmasked tensors alternate in a pattern of period 3 and the missing outputs in one of period 5, so both forms of each
  fall on either side of every 64-item boundary; a k and a cout that are not multiples of 8 are among the shapes."""
  rs = np.random.RandomState(seed)
  out = []
  for i in range(count):
    k, cout = PACK_SHAPES[(i * 7 + seed) % len(PACK_SHAPES)]
    w = rs.randn(k, cout).astype(np.float32)
    mask = (rs.rand(k, cout) < 0.3).astype(np.float32) if i % 3 != 1 else None
    out.append((w, mask, i % 5 != 2, i % 5 != 4))
  return out


def bn_infer_items(count, seed):
  """``count`` frozen batch norms of mixed c as NumPy fp32 (gamma, beta, moving_mean, moving_variance, eps); c = 520 and
  2048 span several 256-thread workgroups."""
  rs = np.random.RandomState(seed)
  out = []
  for i in range(count):
    c = (64, 520, 8, 2048, 3, 256, 257)[(i * 3 + seed) % 7]
    out.append(((rs.rand(c) + 0.5).astype(np.float32), rs.randn(c).astype(np.float32), rs.randn(c).astype(np.float32),
                (rs.rand(c) * 2).astype(np.float32), 1e-3 if i % 2 else 1e-5))
  return out


def bn_infer_ref(gamma, beta, mean, var, eps):
  """The header's formula in float64: scale = gamma / sqrt(var + eps), shift = beta - mean * scale (eps = the fp32 value
  the library receives) -> (scale, shift, bound on scale, bound on shift).  The kernel rounds invstd, the product
  gamma * invstd, mean * scale and the difference to fp32 (4 roundings of 2^-24 each on the magnitudes below, and
  `beta - mean * scale` may or may not be contracted), hence 1e-6 of the magnitudes of the terms."""
  g, b, mu, v = (np.asarray(a, np.float64) for a in (gamma, beta, mean, var))
  scale = g / np.sqrt(v + np.float64(np.float32(eps)))
  shift = b - mu * scale
  return scale, shift, 1e-6 * np.abs(scale), 1e-6 * (np.abs(b) + np.abs(mu * scale))


TOPK_N = (1, 31, 33, 1000, 4097, 50021, 65, 300007, 12345, 7)


def topk_items(count, seed):
  """``count`` layers of mixed n (1 ... 300 007, none a multiple of 32) as (scores fp32 NumPy, n_keep): n_keep = 0 and
  n_keep = n among them, and scores quantised to a few dozen values so that ties straddle the threshold.  The 300 007
  element layer appears once per call."""
  rs = np.random.RandomState(seed)
  out = []
  for i in range(count):
    n = TOPK_N[(i * 3 + seed) % len(TOPK_N)]
    if n == 300007 and any(s.size == n for s, _ in out):
      n = 257
    s = (rs.randint(0, 50, size=n) / 7.0).astype(np.float32) if i % 4 != 3 else rs.randn(n).astype(np.float32)
    keep = (0, n, n // 2, (n * 7) // 10, 1)[i % 5]
    out.append((s, min(keep, n)))
  return out


def topk_ref(score, n_keep):
  """0/1 fp32 mask of the n_keep largest scores, ties by lower index (oracle.rigl_oracle.topk_order)."""
  from oracle import rigl_oracle as O      # pylint: disable=import-outside-toplevel
  ref = np.zeros(score.size, np.float32)
  ref[O.topk_order(score)[:n_keep]] = 1
  return ref
