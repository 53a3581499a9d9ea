"""Exact-integer operands, expected BITS and guard bands for the K1 conv kernels -- TEST INFRASTRUCTURE, never imported
by the product.

With operands that are small integers times a power-of-two unit, and sum|a||b| of every output at most 2^24 units, every
product and every partial sum of a bf16-in / fp32-accumulate (or fp32-in) dot product is exact in fp32 -- in any order, on
any tile shape, under any split.  A kernel's result then has no tolerance at all: the only freedom left is its one
documented final rounding, so every body under every selection knob must produce the same bits, and those bits are
computed here from tests/convref.py's fp64 result (exact for these inputs) by integer arithmetic on the fp32 pattern.

  plan(case, regime, masked)       amplitudes / densities chosen from the SHAPE (never from what a kernel returns)
  operands(case, seed, regime)     x, dy, w, addend (+ the 80 %-off mask of every second seed, as k1_check.run_case)
  reference(op, want)              convref's fp64 run and its |.| run (= sum|a||b| per output element)
  check_conditions(op, ref, ab)    the input conditions of the regime, asserted on the reference before any kernel runs
  rne_bits / expect_*              the documented arithmetic of include/rigl_hip.h, one function per form
  guarded(shape, dtype, device)    an output carved from the middle of a sentinel-filled buffer + its checker

Two regimes per case:
  'low'    nothing rounds anywhere: |y|, |dx| <= 256 units (exactly bf16), and per output channel sum|y| and sum y^2 over all
           rows <= 2^24 units, so ANY partition into statistics parts sums exactly in fp32 and the partials must add up to
           the exact totals.
  'round'  outputs of std 300 .. 1000 units: a value in the binade [2^(8+j), 2^(9+j)) units is an exact bf16 tie with
           probability 2^-(j+1), so >= 5 % of y and of dx are ties (>= 2 % each way) -- round-to-nearest-even, round-half-away,
           truncation and a double rounding all give different bits there.

The rounding functions take NumPy arrays or torch tensors (the same integer expressions; the GPU runner keeps the
batch-128 tensors on the device).  torch's own bf16 conversion is never the judge: tests/test_exactref_cpu.py pins the
integer arithmetic against hand-written ties.
"""
import math
import types

import numpy as np
import torch

from tests import convref

LIMIT = 2 ** 24                           # integers up to here are exact in fp32
SENTINEL16 = 0x7FA5                       # tests/test_glue_edges_gpu.py's: a bf16 NaN no kernel here produces
SENTINEL32 = 0x7FA5A5A5
GUARD_ROWS = 512
FUSED_SCALES = (0.5, -0.5, 1.0, -1.0, 2.0, -2.0)


# ----------------------------------------------------------------------------------------------------------------------
# bf16 rounding as integer arithmetic on the fp32 bit pattern (NumPy arrays or torch tensors)
# ----------------------------------------------------------------------------------------------------------------------
def _is_torch(a):
  return isinstance(a, torch.Tensor)


def f32_pattern(a):
  """Exact values (fp64 / fp32, finite) -> their fp32 bit patterns as int64 in [0, 2^32); asserts that fp32 holds them."""
  if _is_torch(a):
    f = a.to(torch.float32) + 0.0                  # (-0 -> +0: an exact zero is +0)
    assert bool(torch.isfinite(f).all()) and bool((f.double() == a.double()).all()), 'value not exact in fp32'
    return f.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
  a = np.asarray(a)
  f = a.astype(np.float32) + np.float32(0.0)
  assert np.isfinite(f).all() and (f.astype(np.float64) == a.astype(np.float64)).all(), 'value not exact in fp32'
  return f.view(np.uint32).astype(np.int64)


def round_pattern(u, drop, mode='rne'):
  """Drop the low ``drop`` bits of fp32 patterns (int64): 'rne' nearest, ties to even; 'rha' nearest, ties away from zero;
  'trunc' toward zero.  Sign-magnitude patterns: adding to the pattern rounds the magnitude, a carry moves the exponent."""
  if mode == 'trunc':
    return (u >> drop) << drop
  half = 1 << (drop - 1)
  if mode == 'rha':
    return ((u + half) >> drop) << drop
  assert mode == 'rne'
  return ((u + (half - 1) + ((u >> drop) & 1)) >> drop) << drop


def rne_bits(a, mode='rne'):
  """bf16 bit patterns (int64 in [0, 65536)) of exact values under one rounding; 'rne' is the documented one."""
  return round_pattern(f32_pattern(a), 16, mode) >> 16


def double_rounded_bits(a, width=13):
  """A hand-off through a narrower intermediate: first to ``width`` dropped bits (13 = an fp16-wide, 10-bit mantissa), then
  to bf16, both nearest-even -- a mutant for the CPU tests, no kernel's documented arithmetic."""
  return round_pattern(round_pattern(f32_pattern(a), width), 16) >> 16


def bits_value(b):
  """bf16 bit patterns -> their values as fp64."""
  if _is_torch(b):
    v = b.to(torch.int64) << 16
    return torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32).view(torch.float32).double()
  return (np.asarray(b).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def got_bits(t):
  """A bf16 tensor's bit patterns as int64 in [0, 65536) / an fp32 tensor's as int64 in [0, 2^32)."""
  if t.dtype == torch.bfloat16:
    return t.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF
  assert t.dtype == torch.float32
  return t.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def _maximum0(a):
  return torch.clamp(a, min=0) if _is_torch(a) else np.maximum(a, 0)


def _where(c, a, b):
  return torch.where(c, a, b) if _is_torch(a) else np.where(c, a, b)


# ---- one function per documented arithmetic (include/rigl_hip.h, rigl_amd/ops.py docstrings) ---------------------------
def expect_plain(exact):
  """fwd, dgrad, bwd_grid: bf16_rne(exact)."""
  return rne_bits(exact)


def expect_acc(exact, addend):
  """dgrad_acc, bwd, bwd_masked, bwd_sub: bf16(bf16(dgrad) + addend) -- the addend (exact bf16 values, already scattered /
  masked by the caller) meets the ROUNDED gradient, and the sum (exact in fp32, asserted) is rounded once more."""
  return rne_bits(bits_value(rne_bits(exact)) + addend)


def expect_relu(exact):
  """conv_fwd_relu: bf16(max(conv, 0)), +0 for every non-positive value."""
  return rne_bits(_maximum0(exact) + 0.0)


def expect_gate(exact, x):
  """conv_bwd_relu / relu_bwd: bf16(dgrad) * [x > 0], +0 where the gate is shut."""
  b = rne_bits(exact)
  return _where(x > 0, b, b * 0)


def expect_bn_apply(v, scale, shift, residual=None, relu=False):
  """bn_apply / the BN-on-load operand: bf16(relu?(fma(v, scale, shift) (+ residual))) over the channel (last) axis; for the
  operands made here (scale in +-1/2, +-1, +-2, integer shifts) the fma and the sum are exact, so one rounding is left."""
  t = v * scale + shift
  if residual is not None:
    t = t + residual
  if relu:
    t = _maximum0(t) + 0.0
  return rne_bits(t)


def expect_eval(exact, scale, shift, residual=None, relu=False):
  """The eval epilogue (conv_fwd with scale_shift): the header pins it as "bit-identical to rigl_masked_conv2d_fwd followed by
  rigl_bn_apply", so the conv result is rounded to bf16 BEFORE the frozen batch norm -- a stated double rounding:
  bf16(relu?(fma(bf16(conv), scale, shift) (+ residual)))."""
  return expect_bn_apply(bits_value(rne_bits(exact)), scale, shift, residual, relu)


# ----------------------------------------------------------------------------------------------------------------------
# operands
# ----------------------------------------------------------------------------------------------------------------------
def _e2(a):
  """E[v^2] of v uniform on +-{1 .. a}."""
  return (a + 1) * (2 * a + 1) / 6.0


def geometry(case, depthwise=False):
  """Reduction lengths of the three products: K (fwd), Kd (dgrad, the mean number of terms of a dX element), R (wgrad)."""
  N, H, W, Cin, Cout, k, stride, pt, pl, Ho, Wo = case
  fan = 1 if depthwise else Cin
  fan_d = 1 if depthwise else Cout
  # (a strided 1x1 conv reaches only the pixels of its own grid: Kd counts the terms of those, the others are exact zeros)
  return dict(K=k * k * fan, Kd=fan_d * max(1.0, k * k / float(stride * stride)), Kd_max=-(-k // stride) ** 2 * fan_d, R=N * Ho * Wo)


def plan(case, regime, masked, depthwise=False):
  """Amplitudes a* (values uniform on +-{1 .. a}) and densities p* (Bernoulli) of x, dy, w for one case: from the shape alone.

  Both regimes: the weight-gradient sum has R = N Ho Wo terms of |x||dy| each, so ax * ad * R <= 2^24 picks the amplitudes of
  x and dy (at most +-3 where R reaches 1.6 M rows); the weights appear in neither that sum nor its bound.
  'round': the std of y is sqrt(K px E[x^2] pw E[w^2]), of dx sqrt(Kd pd E[dy^2] pw E[w^2]); the densities of x / dy level
  K px E[x^2] with Kd pd E[dy^2], then aw (<= 255) puts both stds at TARGET_STD = 600 units (the tie share peaks there,
  at 22 %: a strided 1x1 dgrad, three quarters of whose dX are structural zeros, still has 5 %).
  'low': about M_LOW = 16 weights per output column are non-zero (+-1, +-2) and px, pd keep E[y^2], E[dx^2] below
  min(400, 2^22 / rows): |y| <= 256 is then 12 sigma away and sum y^2 over the rows is a quarter of 2^24 in expectation.
  (sum|y| <= sum y^2 for integers.)"""
  g = geometry(case, depthwise)
  K, Kd, R = g['K'], g['Kd'], g['R']
  ax, ad = next(((a, b) for a, b in ((3, 3), (3, 2), (2, 2), (2, 1), (1, 1)) if a * b * R <= LIMIT), (1, 1))
  keep = 0.2 if masked else 1.0                    # what the 1-bit mask leaves of w
  if regime == 'round':
    ex, ed = K * _e2(ax), Kd * _e2(ad)
    px, pd = min(1.0, ed / ex), min(1.0, ex / ed)
    c2 = TARGET_STD ** 2 / min(ex, ed)             # = pw_eff E[w^2] wanted
    pw = 1.0
    aw = int(round(math.sqrt(3.0 * c2 / keep)))
    aw = max(1, min(AW_MAX, aw))
    if aw == 1 and keep * 1.0 > c2:                # even +-1 everywhere is too much: thin the weights out
      pw = c2 / keep
  else:
    assert regime == 'low'
    ax, ad, aw = min(ax, 2), min(ad, 2), 2
    m = min(K, M_LOW)
    pw = min(1.0, m / (K * keep))
    pw_eff = pw * keep
    ty, td = min(400.0, LIMIT / 4.0 / R), 400.0
    px = min(1.0, ty / (K * pw_eff * _e2(aw) * _e2(ax)))
    pd = min(1.0, td / (Kd * pw_eff * _e2(aw) * _e2(ad)))
  return dict(ax=ax, ad=ad, aw=aw, px=px, pd=pd, pw=pw, keep=keep, aadd=256 if regime == 'round' else 64)


TARGET_STD = 600.0
AW_MAX = 255                              # every integer up to 255 has 8 significant bits: exact in bf16
M_LOW = 16


def expected_moments(case, p, depthwise=False):
  """E[y^2], E[dx^2] (units^2) under plan ``p``: what the generator aims at, for the checks that do not run the reference."""
  g = geometry(case, depthwise)
  cw = p['pw'] * p['keep'] * _e2(p['aw'])
  return dict(y2=g['K'] * p['px'] * _e2(p['ax']) * cw, dx2=g['Kd'] * p['pd'] * _e2(p['ad']) * cw)


def worst_case(case, p, depthwise=False):
  """max sum|a||b| (units) if every element sat at its amplitude and every position were taken: y, dx, dw."""
  g = geometry(case, depthwise)
  return dict(y=g['K'] * p['ax'] * p['aw'], dx=g['Kd_max'] * p['ad'] * p['aw'], dw=g['R'] * p['ax'] * p['ad'])


def _ints(shape, amp, dens, gen, device):
  """Integers uniform on +-{1 .. amp}, present with probability ``dens``, as fp32."""
  mag = torch.randint(1, amp + 1, shape, generator=gen, device=device, dtype=torch.int16)
  sgn = torch.randint(0, 2, shape, generator=gen, device=device, dtype=torch.int16) * 2 - 1
  v = (mag * sgn).float()
  if dens < 1.0:
    v = v * (torch.rand(shape, generator=gen, device=device) < dens)
  return v + 0.0                                   # (no -0 among the operands)


def units(seed):
  """Power-of-two units 2^-j of x, w, dy -- j varies with the seed and is not always 1."""
  jx, jw, jd = seed % 3, (seed // 3) % 4, (seed // 2) % 3 + 1
  return 2.0 ** -jx, 2.0 ** -jw, 2.0 ** -jd


def operands(case, seed, regime, device='cpu', depthwise=False):
  """The operands of one case: fp32 tensors holding integers times the units (every value exact in bf16).  ``w`` is the
  weight BEFORE the mask [k, k, Cin, Cout] (depthwise: [k, k, C]); ``m01`` the 0/1 mask of every second seed (None: dense);
  ``wm`` = mask * w, what the kernels must see; ``add`` the dgrad addend in units of dx."""
  N, H, W, Cin, Cout, k, stride, pt, pl, Ho, Wo = case
  masked = (seed % 2 == 1) and not depthwise
  p = plan(case, regime, masked, depthwise)
  ux, uw, ud = units(seed)
  gen = torch.Generator(device=device).manual_seed(seed * 2 + (regime == 'round'))
  x = _ints((N, H, W, Cin), p['ax'], p['px'], gen, device) * ux
  dy = _ints((N, Ho, Wo, Cout), p['ad'], p['pd'], gen, device) * ud
  wshape = (k, k, Cin) if depthwise else (k, k, Cin, Cout)
  w = _ints(wshape, p['aw'], p['pw'], gen, device) * uw
  m01 = (torch.rand(wshape, generator=gen, device=device) < 0.2).float() if masked else None
  wm = (w * m01 + 0.0) if masked else w
  add = _ints((N, H, W, Cin), p['aadd'], 0.75, gen, device) * (ud * uw)
  return types.SimpleNamespace(case=case, seed=seed, regime=regime, depthwise=depthwise, plan=p, x=x, dy=dy, w=w, m01=m01, wm=wm,
                               add=add, ux=ux, uw=uw, ud=ud, uy=ux * uw, udx=ud * uw, udw=ux * ud, gen=gen)


def fused_params(op, c, unit, seed):
  """Per-channel scale (+-1/2, +-1, +-2) and integer shift (in ``unit``) for the fused forms: fp32 [2, c] on op.x's device."""
  gen = torch.Generator(device='cpu').manual_seed(seed)
  sc = torch.tensor(FUSED_SCALES)[torch.randint(0, len(FUSED_SCALES), (c,), generator=gen)]
  sh = torch.randint(-2, 3, (c,), generator=gen).float() * unit
  return torch.stack([sc, sh]).contiguous().to(op.x.device)


def reference(op, want=('y', 'dx', 'dw')):
  """(ref, ab): convref's fp64 run on the operands and on their absolute values (ab[.] = sum|a||b| per element)."""
  N, H, W, Cin, Cout, k, stride, pt, pl, Ho, Wo = op.case
  f = convref.depthwise_fp64 if op.depthwise else convref.conv_fp64
  ref = f(op.x, op.wm, op.dy, stride, pt, pl, Ho, Wo, want)
  ab = f(op.x.abs(), op.wm.abs(), op.dy.abs(), stride, pt, pl, Ho, Wo, want)
  return ref, ab


def tie_shares(v, unit):
  """Shares of the values (integers times ``unit``) that are exact bf16 ties: (all, rounding up in magnitude, down to even)."""
  u = f32_pattern(v)
  tie = (u & 0xFFFF) == 0x8000
  up = tie & (((u >> 16) & 1) == 1)
  n = float(u.numel() if _is_torch(u) else u.size)
  return float(tie.sum()) / n, float(up.sum()) / n, float((tie & ~up).sum()) / n


def check_conditions(op, ref, ab):
  """The input conditions of the regime, asserted on the reference: properties of the operands, not of any kernel.
  Returns the figures (for the verdict line)."""
  fig = {}
  for name, unit in (('y', op.uy), ('dx', op.udx), ('dw', op.udw)):
    if name not in ref:
      continue
    r = ref[name] / unit
    assert bool((r == r.round()).all()), '%s: the fp64 reference is not an integer multiple of the unit' % name
    fig['sum_ab_' + name] = float(ab[name].max()) / unit
    assert fig['sum_ab_' + name] <= LIMIT, '%s: max sum|a||b| = %g units > 2^24' % (name, fig['sum_ab_' + name])
  for name, unit in (('y', op.uy), ('dx', op.udx)):
    if name not in ref:
      continue
    r = ref[name] / unit
    if op.regime == 'low':
      fig['max_' + name] = float(r.abs().max())
      assert fig['max_' + name] <= 256, '%s: |%s| = %g units > 256 in the low regime' % (name, name, fig['max_' + name])
      if name == 'y':
        r2 = r.reshape(-1, r.shape[-1])
        fig['sum_abs_y'], fig['sum_y2'] = float(r2.abs().sum(0).max()), float((r2 * r2).sum(0).max())
        assert fig['sum_abs_y'] <= LIMIT and fig['sum_y2'] <= LIMIT, 'low regime: per-channel sum|y| / sum y^2 over 2^24 units'
    else:
      t, up, dn = tie_shares(ref[name], unit)
      fig['ties_' + name] = (round(t, 4), round(up, 4), round(dn, 4))
      fig['std_' + name] = float(r.std())
      assert t >= 0.05 and up >= 0.02 and dn >= 0.02, \
          'round regime: %s has %.2f %% exact bf16 ties (%.2f %% up, %.2f %% to even) at std %.0f units; need 5 / 2 / 2' % (
              name, 100 * t, 100 * up, 100 * dn, fig['std_' + name])
  return fig


# ----------------------------------------------------------------------------------------------------------------------
# comparison and guard bands
# ----------------------------------------------------------------------------------------------------------------------
def assert_bits(name, got, want):
  """``got`` (bit patterns of a kernel's output, got_bits) == ``want`` (expected patterns), elementwise; the message names
  the count and the first flat indices of the wrong elements (the index pattern locates the tile)."""
  if _is_torch(got):
    bad = got.reshape(-1) != want.reshape(-1)
    n = int(bad.sum())
    if n:
      idx = bad.nonzero().reshape(-1)[:8]
      raise AssertionError('%s: %d / %d elements differ in bits; first flat indices %s got %s want %s' % (
          name, n, bad.numel(), idx.tolist(), [hex(v) for v in got.reshape(-1)[idx].tolist()],
          [hex(v) for v in want.reshape(-1)[idx].tolist()]))
    return
  got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
  bad = got != want
  if bad.any():
    idx = np.flatnonzero(bad)[:8]
    raise AssertionError('%s: %d / %d elements differ in bits; first flat indices %s got %s want %s' % (
        name, int(bad.sum()), bad.size, idx.tolist(), [hex(int(v)) for v in got[idx]], [hex(int(v)) for v in want[idx]]))


def guarded(shape, dtype, device='cuda:0', guard_rows=GUARD_ROWS):
  """(out, check, buf): ``out`` = a contiguous tensor of ``shape`` carved from the middle of one larger buffer pre-filled with
  the sentinel, at least ``guard_rows`` output rows (of shape[-1] elements) of guard on each side, 256-byte aligned.
  ``check(name)`` asserts that both guards still hold the sentinel (reporting the first touched offset, in elements relative to
  the start of ``out``) and that no element inside still does.  Everything lies inside one live allocation."""
  itype, sent = {torch.bfloat16: (torch.int16, SENTINEL16), torch.float32: (torch.int32, SENTINEL32)}[dtype]
  size = torch.empty((), dtype=dtype).element_size()
  n = 1
  for s in shape:
    n *= int(s)
  per = 256 // size
  g = -(-(guard_rows * int(shape[-1])) // per) * per           # whole 256-byte lines
  buf = torch.full((g + n + g,), sent, dtype=itype, device=device)
  out = buf[g:g + n].view(dtype).view(shape)
  assert out.data_ptr() % 256 == buf.data_ptr() % 256 and out.is_contiguous()

  def check(name):
    for side, part, base in (('in front of', buf[:g], -g), ('behind', buf[g + n:], n)):
      hit = part != sent
      if bool(hit.any()):
        first = int(hit.nonzero()[0])
        raise AssertionError('%s: wrote %s the output: %d guard elements touched, first at offset %d (output holds [0, %d))' % (
            name, side, int(hit.sum()), base + first, n))
    left = buf[g:g + n] == sent
    if bool(left.any()):
      raise AssertionError('%s: %d / %d output elements never written, first at flat index %d' % (
          name, int(left.sum()), n, int(left.nonzero()[0])))

  return out, check, buf
