#!/usr/bin/env python3
"""K1 exact runner (GPU): every conv entry point of the C ABI on tests/exactref.py's integer operands, against the BITS the
documented arithmetic gives for the exact (fp64) result -- no tolerance -- with every output carved out of a sentinel-filled
buffer (guard bands in front and behind, no element left unwritten).

The kernel-selection knobs all have run-time twins (ops.tune_set), so one process walks a case list: per case and regime
('low': nothing rounds, statistics partials add up exactly; 'round': outputs on bf16 ties) the operands and the fp64
reference are made once, the input conditions (sum|a||b| <= 2^24 units, tie shares) are asserted on the reference, and then
every setting of the set must reproduce the same expected bits -- so all bodies are bit-identical to each other as well.

  python tests/k1_exact.py --set small          # k1_check.SMALL_CASES under test_k1_parity_gpu.PP_SETTINGS
  python tests/k1_exact.py --set pp             # ... PP_CASES under the same settings
  python tests/k1_exact.py --set stem | c3 | bs # default, and with the body's knob off
  python tests/k1_exact.py --set rs             # rowstream = 2 / default / 0
  python tests/k1_exact.py --set resnet50 --batch 128      # default and the all-generic setting
  python tests/k1_exact.py --set mobilenet_v1 --batch 128  # default, rowstream = 2, all-generic
  python tests/k1_exact.py --set vgg            # test_vgg_gpu's 3x3 shapes, with and without the fused ReLU
  python tests/k1_exact.py --set dw | dw128     # depthwise: test_k3_k1_gpu's cases / MobileNet-v1's layers at batch 128
  python tests/k1_exact.py --set f32            # the fp32 twin on test_k1_fp32_gpu.KERNEL_CASES, dense and masked
  python tests/k1_exact.py --set wrn | odd      # k1_check.WRN_CASES / ODD_CASES: default and the all-generic setting
  python tests/k1_exact.py --set mlp            # k1_check.MLP_CASES: default (no knob reaches the direct kernels)
  python tests/k1_exact.py --set small --workspace exact   # the same walk on tests/wsguard.py's workspace, once per poison

The small-channel sets (FULL_SETS: wrn, mlp, odd) want dX for EVERY case: where cin or cout is no multiple of 8 it comes from
the direct kernel of conv_ref.hip through ops.conv_dgrad and from the host fallback of ops.conv_bwd (conv_wgrad + conv_dgrad
+ a torch addition of the addend), against the same expected bits.  On these sets no wrapper form is skipped: a form a shape
does not take (statistics, the fused ReLUs, addend_sub, addend_bits, the own-grid backward, the eval epilogue, BN on load)
must be REFUSED as documented -- ValueError / RiglError, (y, None) for the statistics -- with every guarded output handed to it
still all sentinel; lib_forms() says which, read from rigl_amd/ops.py and csrc/conv.hip, and the verdict counts them
("refused").  The older sets run the checks they always ran.  REF_SETS (those three and small) add the direct kernels as
forms of their own -- fwd_ref, dgrad_ref, wgrad_ref through force_ref=True -- once per poison; they accumulate with fmaf in
(r, s, c) order, and on these operands every partial sum is an integer of at most 2^24 units, so any order gives the same bits.

--workspace pool (the default) is the product's grow-only pool.  With --workspace exact every scratch request is carved
exactly as long as the size query said, between two 1 MiB guards, and pre-filled with a poison (0x00, then 0xFF): every
setting of every case runs once per poison against the SAME expected bits (they do not depend on the summation order, so
a layer may split or not), and after every verified output the workspace guards must be intact as well.  The verdict then
carries "workspace": {"mode": "exact", "poisons": [...], "requests": n, "guards": "intact", "max_bytes": b, "max_used": u}
(max_used: the largest high-water mark, one past the last payload byte that differs from the poison -- reported only).

Prints one line per case and regime and a final JSON verdict {"ok": true, "cases": n, "settings": m, "checks": c,
"refused": r, "diff_bits": 0, "guards": "intact", "unwritten": 0, ...}; stops at the first failure with exit code 1.
Test infrastructure: tests/test_k1_exact_gpu.py calls it in a subprocess, each under its own timeout.
"""
import argparse
import ctypes
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests import exactref as E  # noqa: E402
from tests import k1_check  # noqa: E402

DEV = 'cuda:0'
BF, F32 = torch.bfloat16, torch.float32
GENERIC = {'bwd1x1': 0, 'stem_direct': 0, 'wgrad_il': 0, 'c3x3': 0, 'rowstream': 0, 'bwdslice': 0}


def _knobs(env):
  """{'RIGL_PP_FWD': '1'} -> {'pp_fwd': 1}: an environment setting of the parity tests as its run-time twin."""
  return {k[len('RIGL_'):].lower(): int(v) for k, v in env.items()}


def settings_for(name):
  if name in ('small', 'pp'):
    from tests.test_k1_parity_gpu import PP_SETTINGS
    return [_knobs(e) for e in PP_SETTINGS]
  return {'stem': [{}, {'stem_direct': 0}], 'c3': [{}, {'c3x3': 0}], 'bs': [{}, {'bwdslice': 0}],
          'rs': [{'rowstream': 2}, {}, {'rowstream': 0}], 'resnet50': [{}, GENERIC],
          'mobilenet_v1': [{}, {'rowstream': 2}, GENERIC], 'vgg': [{'relu_fuse': 1}, {'relu_fuse': 0}],
          'dw': [{}], 'dw128': [{}], 'f32': [{}],
          # (no knob reaches the direct kernels, which run all but one of mlp's layers)
          'wrn': [{}, GENERIC], 'odd': [{}, GENERIC], 'mlp': [{}]}[name]


def cases_for(name, batch):
  fixed = {'small': k1_check.SMALL_CASES, 'pp': k1_check.PP_CASES, 'stem': k1_check.STEM_CASES, 'c3': k1_check.C3_CASES,
           'rs': k1_check.RS_CASES, 'bs': k1_check.BS_CASES, 'wrn': k1_check.WRN_CASES, 'mlp': k1_check.MLP_CASES,
           'odd': k1_check.ODD_CASES}
  if name in fixed:
    return fixed[name]
  if name == 'resnet50':
    return k1_check.resnet50_shapes(batch)
  if name == 'mobilenet_v1':
    return k1_check.mobilenet_v1_shapes(batch)
  if name == 'vgg':
    from tests.test_vgg_gpu import C3_SHAPES, VGG16_SHAPES
    return [(n, h, w, ci, co, 3, 1, 1, 1, h, w) for n, h, w, ci, co in VGG16_SHAPES + C3_SHAPES]
  if name == 'f32':
    from tests.test_k1_fp32_gpu import KERNEL_CASES
    return [(n, h, w, ci, co, k, s, p, p, ho, wo) for n, h, w, ci, co, k, s, p, ho, wo in KERNEL_CASES]
  from tests import test_k3_k1_gpu as T
  if name == 'dw128':
    return [(batch, hw, hw, c, c, 3, s, 1, 1, (hw - 1) // s + 1, (hw - 1) // s + 1) for hw, c, s in T.MOBILENET_V1_DEPTHWISE]
  assert name == 'dw'
  out = []
  for c in next(m for m in T.test_depthwise_conv.pytestmark if m.name == 'parametrize').args[1]:
    N, H, W, C, k, s = c[:6]
    if len(c) > 6:                                 # TF SAME: out = ceil(in / s), the extra padding at the end
      Ho, Wo = -(-H // s), -(-W // s)
      pt, pl = max((Ho - 1) * s + k - H, 0) // 2, max((Wo - 1) * s + k - W, 0) // 2
    else:
      Ho, Wo, pt, pl = (H - 1) // s + 1, (W - 1) // s + 1, (k - 1) // 2, (k - 1) // 2
    out.append((N, H, W, C, C, k, s, pt, pl, Ho, Wo))
  return out


# Seed = 100 + case index (+ an offset where the input conditions of a case fall short at its own seed).  The two masked
# strided 1x1 cases with few output columns: three quarters of dX are structural zeros, so the tie share of a strided 1x1
# dgrad is a quarter of the 22 % the plan aims at, and with 80 % of 32 / 40 weights per input channel masked off the std of dX
# scatters so much from channel to channel that the share falls under the 5 % bound (fp64 reference on the CPU, 30 odd seeds:
# mean 4.95 % / 5.37 %, lowest 4.4 % / 4.8 %).  One seed on they are dense (30 even seeds: lowest 5.4 %); the masked strided
# 1x1 is PP_CASES' 512 -> 256 layer.
SEED_OFFSET = {('wrn', 3): 1, ('odd', 3): 1}


def seed_for(name, i):
  return 100 + i + SEED_OFFSET.get((name, i), 0)


class Tally:
  checks = 0
  refused = 0                              # forms asserted refused, their outputs left all sentinel


class WS:
  """--workspace exact: the installed tests/wsguard.GuardedWorkspace and the poisons to walk (None: the product's pool)."""
  guard = None
  poisons = ()
  by_form = {}                             # verified output (without its setting) -> [requests, largest declared, largest used]


def _poisons():
  """Once per poison with the guard's poison set (no region is live when it changes); once, with None, on the pool."""
  if WS.guard is None:
    yield None
    return
  for p in WS.poisons:
    WS.guard.check('before poison 0x%02X' % p)
    WS.guard.poison = p
    yield p
  WS.guard.check('after the last poison')


def _ws_check(name):
  if WS.guard is not None:
    for _, nbytes, used in WS.guard.check(name + ' [poison 0x%02X]' % WS.guard.poison):
      t = WS.by_form.setdefault(name.split(' [')[0], [0, 0, 0])
      t[0], t[1], t[2] = t[0] + 1, max(t[1], nbytes), max(t[2], used)


def _g(shape, dtype):
  return E.guarded(shape, dtype, DEV)


def _verify(name, out, check, want):
  """Guards intact, nothing unwritten, and the output's bits == the expected bits."""
  check(name)
  E.assert_bits(name, E.got_bits(out), want)
  _ws_check(name)
  Tally.checks += 1


def _bf(t, what):
  b = t.to(BF)
  assert bool((b.float() == t).all()), '%s: an operand is not exact in bf16' % what
  return b


def _pack(op, ops):
  """bf16 shadows through the product's own pack kernel (mask bits for every second seed), pinned to bf16(mask * w)."""
  k, _, Cin, Cout = op.w.shape
  n = op.w.numel()
  hwio, chk_h, _ = _g((n,), BF)
  ohwi, chk_o, _ = _g((n,), BF)
  bits = ops.mask_pack(op.m01.reshape(-1).contiguous()) if op.m01 is not None else None
  ops.pack_weights(op.w.reshape(-1).contiguous(), bits, k * k * Cin, Cout, hwio, ohwi)
  want = E.rne_bits(op.wm.reshape(-1))
  _verify('pack.hwio', hwio, chk_h, want)
  _verify('pack.ohwi', ohwi, chk_o, want.reshape(k * k * Cin, Cout).t().contiguous())
  return hwio, ohwi, bits


FULL_SETS = ('wrn', 'mlp', 'odd')          # dX wanted for every case; every wrapper form verified or asserted refused
REF_SETS = FULL_SETS + ('small',)          # + the direct kernels (force_ref=True) as forms of their own


def lib_forms(case):
  """What rigl_amd/ops.py and csrc/conv.hip take on a shape (everything else is refused, see run_conv_case):
  ``mfma``     cout % 8 == 0: forward and weight gradient on the MFMA bodies (tiny Cin on the padded-to-4 input, other
               cin % 8 != 0 on the explicit im2col matrix), statistics, the fused ReLU, the eval epilogue (in place or as
               conv + bn_apply, whose channel count must be a multiple of 8); else the direct kernels and no epilogue
  ``mfma_dx``  cin % 8 == cout % 8 == 0: dX on the MFMA bodies, bwd_sub, bwd_relu, the BN-on-load eval forward; else dX from
               the direct kernel and conv_bwd = conv_wgrad + conv_dgrad (+ a torch addition of the addend) on the host
  ``grid``     the own-grid backward: a 1x1 conv without padding whose output grid is every stride-th pixel (stride 1 included)
  ``bits8``    dX has a multiple of 8 elements: an addend mask is one bit per element in whole bytes, and the stand-alone
               rigl_relu_bwd takes n % 8 == 0 only"""
  N, H, W, Cin, Cout, k, stride, pt, pl, Ho, Wo = case
  a, b = Cout % 8 == 0, Cin % 8 == 0
  own = k == 1 and pt == 0 and pl == 0 and Ho == -(-H // stride) and Wo == -(-W // stride)
  return dict(mfma=a, mfma_dx=a and b, grid=own and a and b, bits8=(N * H * W * Cin) % 8 == 0)


def routes(case):
  """Which kernels ORDINARY dispatch (no force_ref) runs a shape on: for the per-case line."""
  f = lib_forms(case)
  cin = case[3]
  body = 'tiny' if cin <= 4 else 'im2col' if cin % 8 else 'mfma'
  return dict(fwd=body if f['mfma'] else 'direct', wgrad=body if f['mfma'] else 'direct',
              dgrad='mfma' if f['mfma_dx'] else 'direct', bwd='one call' if f['mfma_dx'] else 'host fallback')


def expectations(op, ref, full):
  """The expected bits of every form of one case, from the fp64 reference ``ref`` (on op.x's device: the CPU tests run this
  too).  ``full``: dX for every shape and the fused forms on every shape (FULL_SETS); else what the older sets check."""
  N, H, W, Cin, Cout, k, stride, pt, pl, Ho, Wo = op.case
  dev = op.x.device
  f = lib_forms(op.case)
  e = types.SimpleNamespace(forms=f)
  e.has_dx = 'dx' in ref
  e.want_y, e.want_dw = E.expect_plain(ref['y']), E.f32_pattern(ref['dw'].reshape(-1))
  e.want_yr = E.expect_relu(ref['y'])
  y2d = ref['y'].reshape(-1, Cout)
  e.tot = (y2d.sum(0), (y2d * y2d).sum(0)) if op.regime == 'low' else None
  if e.has_dx:
    e.want_dx, e.want_dxa = E.expect_plain(ref['dx']), E.expect_acc(ref['dx'], op.add.double())
    e.want_gate = E.expect_gate(ref['dx'], op.x)
    e.addc = op.add[:, ::2, ::2, :].contiguous().to(BF)
    full_add = torch.zeros_like(op.add)
    full_add[:, ::2, ::2, :] = op.add[:, ::2, ::2, :]
    e.want_sub = E.expect_acc(ref['dx'], full_add.double())
    del full_add
    n_in = op.add.numel()
    m01 = torch.rand(n_in, generator=op.gen, device=dev) < 0.4
    e.abits = torch.zeros(-(-n_in // 8), dtype=torch.uint8, device=dev)
    if f['bits8']:
      for j in range(8):
        e.abits |= (m01.view(-1, 8)[:, j].to(torch.uint8) << j)
    e.want_msk = E.expect_acc(ref['dx'], torch.where(m01.view(op.add.shape), op.add, torch.zeros_like(op.add)).double())
    del m01
    e.grid = f['grid'] if full else k == 1 and stride > 1 and pt == 0 and pl == 0 and Ho == -(-H // stride) and Wo == -(-W // stride)
    e.want_grid = E.expect_plain(ref['dx'][:, ::stride, ::stride, :].contiguous()) if e.grid else None
  e.fused = full or (k == 1 and stride == 1 and Cout % 8 == 0 and e.has_dx)
  if e.fused:
    # the eval epilogue: per-channel scale in +-1/2, +-1, +-2, integer shifts, an integer residual -- the fma is exact
    e.ss = E.fused_params(op, Cout, op.uy, op.seed + 7)
    res = E._ints((N, Ho, Wo, Cout), 64, 0.75, op.gen, dev) * op.uy
    e.res_b = _bf(res, 'residual')
    e.want_ev = {(r, rl): E.expect_eval(ref['y'], e.ss[0].double(), e.ss[1].double(), res.double() if r else None, rl)
                 for r, rl in ((True, True), (False, False))}
    # BN on load: a = bf16(relu(fma(x, scale, shift))) (exact: half-units of x), then the conv of it
    e.ssi = E.fused_params(op, Cin, op.ux, op.seed + 11)
    e.saved = torch.cat([torch.zeros_like(e.ssi), e.ssi]).contiguous()      # [4, Cin]: rows 2-3 = scale, shift
    e.want_a = E.expect_bn_apply(op.x.double(), e.ssi[0].double(), e.ssi[1].double(), None, True)
    a_val = E.bits_value(e.want_a).reshape(op.x.shape)
    from tests import convref
    ya = convref.conv_fp64(a_val, op.wm, op.dy, stride, pt, pl, Ho, Wo, ('y',))['y']
    ya_ab = convref.conv_fp64(a_val.abs(), op.wm.abs(), op.dy, stride, pt, pl, Ho, Wo, ('y',))['y']
    assert float(ya_ab.max()) / (op.uy / 2) <= E.LIMIT, 'BN on load: sum|a||w| over 2^24 half-units'
    e.want_ya = E.expect_plain(ya)
    e.want_ya_ev = E.expect_eval(ya, e.ss[0].double(), e.ss[1].double(), res.double(), True)
  return e


def _refused(name, exc, call, *bufs):
  """The documented refusal of a form on a shape: ``call`` raises ``exc`` (ValueError from the wrapper, RiglError from the
  library) and every guarded output handed to it is still all sentinel, guards and payload: nothing was launched on it."""
  try:
    call()
  except exc:
    pass
  else:
    raise AssertionError('%s: not refused (%s expected)' % (name, getattr(exc, '__name__', exc)))
  _untouched(name, *bufs)
  Tally.refused += 1


def _untouched(name, *bufs):
  for b in bufs:
    sent = E.SENTINEL16 if b.dtype == torch.int16 else E.SENTINEL32
    hit = b != sent
    if bool(hit.any()):
      raise AssertionError('%s: refused, but %d elements of an output buffer were written, first at %d of %d' % (
          name, int(hit.sum()), int(hit.nonzero()[0]), b.numel()))


def _masked_form_runs(ops, case):
  """Does rigl_masked_conv2d_bwd_masked have a kernel for this shape under the knobs in force?  The library's own query with
  "rs_masked_addend" = 2 (every legal layer, not only those it recommends the hand-over for), on a fresh descriptor."""
  N, H, W, Cin, Cout, k, stride, pt, pl, Ho, Wo = case
  ops.tune_set('rs_masked_addend', 2)
  try:
    return ops.conv_bwd_takes_masked_addend(ops.conv_desc(N, H, W, Cin, Cout, k, k, stride, pt, pl, Ho, Wo))
  finally:
    ops.tune_unset('rs_masked_addend')


def run_conv_case(case, seed, regime, settings, full=False, ref_forms=False):
  """``full`` (FULL_SETS): dX is wanted whatever cin (from the direct kernel and the host fallbacks of ops.conv_dgrad /
  ops.conv_bwd where the MFMA dgrad does not apply), and every wrapper form the older sets skip on a shape either gives the
  expected bits or its documented refusal is asserted with the outputs left all sentinel (lib_forms says which).
  ``ref_forms`` (REF_SETS): the three direct kernels through force_ref=True, once per poison (no knob reaches them)."""
  from rigl_amd import _lib, ops
  lib = _lib.load()
  RiglError = _lib.RiglError
  N, H, W, Cin, Cout, k, stride, pt, pl, Ho, Wo = case
  op = E.operands(case, seed, regime, DEV)
  x, dy, add = _bf(op.x, 'x'), _bf(op.dy, 'dy'), _bf(op.add, 'addend')
  hwio, ohwi, _ = _pack(op, ops)
  d = ops.conv_desc(N, H, W, Cin, Cout, k, k, stride, pt, pl, Ho, Wo)
  has_dx = full or Cin % 8 == 0
  assert has_dx or not ref_forms
  ref, ab = E.reference(op, ('y', 'dx', 'dw') if has_dx else ('y', 'dw'))
  fig = E.check_conditions(op, ref, ab)
  del ab
  n_w = k * k * Cin * Cout
  # ---- the expected bits, once per case -------------------------------------------------------------------------------
  e = expectations(op, ref, full)
  del ref
  f = e.forms
  if full:
    fig['route'] = routes(case)
    assert ops.mfma_supported(d) == f['mfma'] and ops.mfma_dgrad_supported(d) == f['mfma_dx']
  # ---- every setting must reproduce them ------------------------------------------------------------------------------
  for _ in _poisons():
    if ref_forms:
      y, chk, _ = _g((N, Ho, Wo, Cout), BF)
      assert ops.conv_fwd(d, x, ohwi, y=y, force_ref=True) is y
      _verify('fwd_ref', y, chk, e.want_y)
      dx, chk, _ = _g((N, H, W, Cin), BF)
      ops.conv_dgrad(d, dy, hwio, dx=dx, force_ref=True)
      _verify('dgrad_ref', dx, chk, e.want_dx)
      dw, chk, _ = _g((n_w,), F32)
      ops.conv_wgrad(d, x, dy, dw=dw, force_ref=True)
      _verify('wgrad_ref', dw, chk, e.want_dw)
      del y, dx, dw
    for knobs in settings:
      _run_setting(ops, lib, RiglError, d, case, knobs, full, has_dx, e, x, dy, add, hwio, ohwi, n_w)
  torch.cuda.synchronize()
  return fig


def _run_setting(ops, lib, RiglError, d, case, knobs, full, has_dx, e, x, dy, add, hwio, ohwi, n_w):
  N, H, W, Cin, Cout, k, stride, pt, pl, Ho, Wo = case
  f, tot = e.forms, e.tot
  tag = lambda s: '%s [%s]' % (s, ' '.join('%s=%d' % kv for kv in sorted(knobs.items())) or 'default')   # noqa: E731
  try:
    for key, v in knobs.items():
      ops.tune_set(key, v)
    y, chk, _ = _g((N, Ho, Wo, Cout), BF)
    ops.conv_fwd(d, x, ohwi, y=y)
    _verify(tag('fwd'), y, chk, e.want_y)
    if Cout % 8 == 0:
      parts = int(lib.rigl_conv2d_stats_parts(ctypes.byref(d)))
      y2, chk, _ = _g((N, Ho, Wo, Cout), BF)
      part, chkp, _ = _g((parts, 2, Cout), F32)
      _, p2 = ops.conv_fwd(d, x, ohwi, y=y2, stats=True, part=part)
      assert p2 is part
      _verify(tag('fwd_stats.y'), y2, chk, e.want_y)
      chkp(tag('fwd_stats.part'))
      if tot is not None:
        s = part.double().sum(0)
        assert torch.equal(s[0], tot[0]), tag('fwd_stats: the partials do not add up to the exact sum y')
        assert torch.equal(s[1], tot[1]), tag('fwd_stats: the partials do not add up to the exact sum y^2')
      Tally.checks += 1
      del y2, part
      yr, chk, _ = _g((N, Ho, Wo, Cout), BF)
      ops.conv_fwd_relu(d, x, ohwi, y=yr)
      _verify(tag('fwd_relu'), yr, chk, e.want_yr)
      yr, chk, _ = _g((N, Ho, Wo, Cout), BF)
      ops.relu_fwd(y, y=yr)
      _verify(tag('relu_fwd(fwd)'), yr, chk, e.want_yr)
      del yr
    elif full:
      # cout % 8 != 0: the direct forward has no statistics epilogue -- (y, None), the caller's part buffer untouched -- and
      # no fused ReLU (RIGL_EUNSUPPORTED)
      assert int(lib.rigl_conv2d_stats_parts(ctypes.byref(d))) == 0
      y2, chk, _ = _g((N, Ho, Wo, Cout), BF)
      part, _, pbuf = _g((1, 2, Cout), F32)
      y3, p2 = ops.conv_fwd(d, x, ohwi, y=y2, stats=True, part=part)
      assert y3 is y2 and p2 is None, tag('fwd_stats: (y, None) expected where the MFMA path does not apply')
      _verify(tag('fwd_stats.y (no statistics)'), y2, chk, e.want_y)
      _untouched(tag('fwd_stats.part (no statistics)'), pbuf)
      Tally.refused += 1
      yr, _, ybuf = _g((N, Ho, Wo, Cout), BF)
      _refused(tag('fwd_relu'), RiglError, lambda: ops.conv_fwd_relu(d, x, ohwi, y=yr), ybuf)
      del y2, part, yr
    del y
    dw, chk, _ = _g((n_w,), F32)
    ops.conv_wgrad(d, x, dy, dw=dw)
    _verify(tag('wgrad'), dw, chk, e.want_dw)
    if not has_dx:
      dw, chk, _ = _g((n_w,), F32)
      assert ops.conv_bwd(d, x, dy, hwio, dw, need_dx=False) is None
      _verify(tag('bwd.dw (no dX)'), dw, chk, e.want_dw)
      return
    dx, chk, _ = _g((N, H, W, Cin), BF)
    ops.conv_dgrad(d, dy, hwio, dx=dx)
    _verify(tag('dgrad'), dx, chk, e.want_dx)
    dxg, chkg, gbuf = _g((N, H, W, Cin), BF)
    if f['bits8']:
      ops.relu_bwd(dx, x, dx=dxg)
      _verify(tag('relu_bwd(dgrad)'), dxg, chkg, e.want_gate)
    else:                                            # rigl_relu_bwd: n % 8 == 0 (include/rigl_hip.h)
      _refused(tag('relu_bwd(dgrad)'), RiglError, lambda: ops.relu_bwd(dx, x, dx=dxg), gbuf)
    del dxg
    dx, chk, _ = _g((N, H, W, Cin), BF)
    ops.conv_dgrad(d, dy, hwio, dx=dx, addend=add)
    _verify(tag('dgrad_acc'), dx, chk, e.want_dxa)
    forms = [('bwd', dict(addend=add), e.want_dxa), ('bwd (no addend)', {}, e.want_dx)]
    sub = ('bwd_sub', dict(addend=e.addc, addend_sub=(2, 2)), e.want_sub)
    msk = ('bwd_masked', dict(addend=add, addend_bits=e.abits), e.want_msk)
    refusals = []
    if not full:
      forms.append(sub)
      if ops.conv_bwd_takes_masked_addend(d):
        forms.append(msk)
    else:
      if f['mfma_dx']:
        forms.append(sub)
      else:
        refusals.append((sub, ValueError))           # ops.conv_bwd: addend_sub needs cin % 8 == cout % 8 == 0
      if not f['bits8']:
        refusals.append((msk, ValueError))           # ops.conv_bwd: one bit per element of dX, in whole bytes
      elif _masked_form_runs(ops, case):
        forms.append(msk)
      else:
        refusals.append((msk, RiglError))            # the library: this layer's kernels take no masked addend
    for nm, kw, want in forms:
      dx, chk, _ = _g((N, H, W, Cin), BF)
      dw, chkw, _ = _g((n_w,), F32)
      assert ops.conv_bwd(d, x, dy, hwio, dw, need_dx=True, dx=dx, **kw) is dx
      _verify(tag(nm + '.dx'), dx, chk, want)
      _verify(tag(nm + '.dw'), dw, chkw, e.want_dw)
    for (nm, kw, _), exc in refusals:
      dx, _, xbuf = _g((N, H, W, Cin), BF)
      dw, _, wbuf = _g((n_w,), F32)
      _refused(tag(nm), exc, lambda: ops.conv_bwd(d, x, dy, hwio, dw, need_dx=True, dx=dx, **kw), xbuf, wbuf)
    if f['mfma_dx'] or not full:
      dx, chk, _ = _g((N, H, W, Cin), BF)
      dw, chkw, _ = _g((n_w,), F32)
      ops.conv_bwd_relu(d, x, dy, hwio, dw, dx=dx)
      _verify(tag('bwd_relu.dx'), dx, chk, e.want_gate)
      _verify(tag('bwd_relu.dw'), dw, chkw, e.want_dw)
    else:
      dx, _, xbuf = _g((N, H, W, Cin), BF)
      dw, _, wbuf = _g((n_w,), F32)
      _refused(tag('bwd_relu'), RiglError, lambda: ops.conv_bwd_relu(d, x, dy, hwio, dw, dx=dx), xbuf, wbuf)
    if e.grid:
      dxs, chk, _ = _g((N, Ho, Wo, Cin), BF)
      dw, chkw, _ = _g((n_w,), F32)
      ops.conv_bwd_grid(d, x, dy, hwio, dw, dx=dxs)
      _verify(tag('bwd_grid.dx'), dxs, chk, e.want_grid)
      _verify(tag('bwd_grid.dw'), dw, chkw, e.want_dw)
      del dxs
    elif full:
      dxs, _, xbuf = _g((N, Ho, Wo, Cin), BF)
      dw, _, wbuf = _g((n_w,), F32)
      _refused(tag('bwd_grid'), RiglError, lambda: ops.conv_bwd_grid(d, x, dy, hwio, dw, dx=dxs), xbuf, wbuf)
      del dxs
    del dx, dw
    if not e.fused:
      return
    if f['mfma']:
      for (r, rl), want in e.want_ev.items():
        ye, chk, _ = _g((N, Ho, Wo, Cout), BF)
        ops.conv_fwd(d, x, ohwi, y=ye, scale_shift=e.ss, residual=e.res_b if r else None, relu=rl)
        _verify(tag('fwd_eval(residual=%d, relu=%d)' % (r, rl)), ye, chk, want)
    else:                                            # conv + bn_apply on the host, and rigl_bn_apply takes channels % 8 == 0 only
      ye, _, ybuf = _g((N, Ho, Wo, Cout), BF)
      _refused(tag('fwd_eval'), RiglError,
               lambda: ops.conv_fwd(d, x, ohwi, y=ye, scale_shift=e.ss, residual=e.res_b, relu=True), ybuf)
    if f['mfma_dx']:
      ye, chk, _ = _g((N, Ho, Wo, Cout), BF)
      ops.conv_fwd_bnrelu(d, x, e.ssi, ohwi, None, y=ye, scale_shift=e.ss, residual=e.res_b, relu=True)
      _verify(tag('fwd_bnrelu eval'), ye, chk, e.want_ya_ev)
    else:
      ye, _, ybuf = _g((N, Ho, Wo, Cout), BF)
      _refused(tag('fwd_bnrelu eval'), RiglError,
               lambda: ops.conv_fwd_bnrelu(d, x, e.ssi, ohwi, None, y=ye, scale_shift=e.ss, residual=e.res_b, relu=True), ybuf)
    if ops.conv_fwd_takes_bn_input(d):
      parts = int(lib.rigl_conv2d_stats_parts(ctypes.byref(d)))
      ye, chk, _ = _g((N, Ho, Wo, Cout), BF)
      a_out, chka, _ = _g((N, H, W, Cin), BF)
      part, chkp, _ = _g((parts, 2, Cout), F32)
      ops.conv_fwd_bnrelu(d, x, e.saved, ohwi, a_out, y=ye, stats=True, part=part)
      _verify(tag('fwd_bnrelu.y'), ye, chk, e.want_ya)
      _verify(tag('fwd_bnrelu.a_out'), a_out, chka, e.want_a)
      chkp(tag('fwd_bnrelu.part'))
      del a_out, part
    elif full:
      ye, _, ybuf = _g((N, Ho, Wo, Cout), BF)
      a_out, _, abuf = _g((N, H, W, Cin), BF)
      _refused(tag('fwd_bnrelu (training)'), RiglError, lambda: ops.conv_fwd_bnrelu(d, x, e.saved, ohwi, a_out, y=ye), ybuf, abuf)
      del a_out
    del ye
  finally:
    for key in knobs:
      ops.tune_unset(key)


def run_depthwise_case(case, seed, regime, settings):
  from rigl_amd import _lib, ops
  lib = _lib.load()
  N, H, W, C, _, k, stride, pt, pl, Ho, Wo = case
  op = E.operands(case, seed, regime, DEV, depthwise=True)
  x, dy = _bf(op.x, 'x'), _bf(op.dy, 'dy')
  wd = op.w.reshape(-1).contiguous()                 # fp32 [k, k, C], read directly (these layers are not masked)
  d = ops.conv_desc(N, H, W, C, C, k, k, stride, pt, pl, Ho, Wo)
  ref, ab = E.reference(op)
  fig = E.check_conditions(op, ref, ab)
  del ab
  want_y, want_dx, want_dw = E.expect_plain(ref['y']), E.expect_plain(ref['dx']), E.f32_pattern(ref['dw'].reshape(-1))
  y2d = ref['y'].reshape(-1, C)
  tot = (y2d.sum(0), (y2d * y2d).sum(0)) if regime == 'low' else None
  del ref
  for _ in _poisons():
    y, chk, _ = _g((N, Ho, Wo, C), BF)
    ops.depthwise_fwd(d, x, wd, y=y)
    _verify('depthwise fwd', y, chk, want_y)
    parts = int(lib.rigl_depthwise_conv2d_stats_parts(ctypes.byref(d)))
    if parts > 0:
      y, chk, _ = _g((N, Ho, Wo, C), BF)
      part, chkp, _ = _g((parts, 2, C), F32)
      _, p2 = ops.depthwise_fwd(d, x, wd, stats=True, y=y, part=part)
      assert p2 is part
      _verify('depthwise fwd_stats.y', y, chk, want_y)
      chkp('depthwise fwd_stats.part')
      if tot is not None:
        s = part.double().sum(0)
        assert torch.equal(s[0], tot[0]), 'depthwise fwd_stats: the partials do not add up to the exact sum y'
        assert torch.equal(s[1], tot[1]), 'depthwise fwd_stats: the partials do not add up to the exact sum y^2'
      Tally.checks += 1
    dx, chk, _ = _g((N, H, W, C), BF)
    ops.depthwise_dgrad(d, dy, wd, dx=dx)
    _verify('depthwise dgrad', dx, chk, want_dx)
    dw, chk, _ = _g((k * k * C,), F32)
    ops.depthwise_wgrad(d, x, dy, dw)
    _verify('depthwise wgrad', dw, chk, want_dw)
  torch.cuda.synchronize()
  return fig


def run_f32_case(case, seed, regime, settings):
  """The fp32 twin: the same integers as fp32 tensors, the fp32 master weights with and without the mask bitmap; every
  output is fp32 and exact, dX + addend included (one exact sum)."""
  from rigl_amd import ops
  N, H, W, Cin, Cout, k, stride, pt, pl, Ho, Wo = case
  op = E.operands(case, seed | 1, regime, DEV)       # (an odd seed: the operands carry a mask; dense = the same w unmasked)
  d = ops.conv_desc(N, H, W, Cin, Cout, k, k, stride, pt, pl, Ho, Wo)
  bits = ops.mask_pack(op.m01.reshape(-1).contiguous())
  n_w = op.w.numel()
  fig = {}
  for nm, mb, wm in (('masked', bits, op.wm), ('dense', None, op.w)):
    op.wm = wm
    ref, ab = E.reference(op)
    if nm == 'masked':
      fig = E.check_conditions(op, ref, ab)
    else:
      for key, unit in (('y', op.uy), ('dx', op.udx)):
        assert float(ab[key].max()) / unit <= E.LIMIT, 'f32 dense: sum|a||b| over 2^24 units'
    del ab
    for _ in _poisons():
      y, chk, _ = _g((N, Ho, Wo, Cout), F32)
      ops.conv_fwd_f32(d, op.x, op.w.reshape(-1), mb, y=y)
      _verify('fwd_f32 ' + nm, y, chk, E.f32_pattern(ref['y']))
      dx, chk, _ = _g((N, H, W, Cin), F32)
      dw, chkw, _ = _g((n_w,), F32)
      ops.conv_bwd_f32(d, op.x, op.dy, op.w.reshape(-1), mb, dw, need_dx=True, addend=op.add, dx=dx)
      _verify('bwd_f32.dx ' + nm, dx, chk, E.f32_pattern(ref['dx'] + op.add.double()))
      _verify('bwd_f32.dw ' + nm, dw, chkw, E.f32_pattern(ref['dw'].reshape(-1)))
      dx, chk, _ = _g((N, H, W, Cin), F32)
      ops.conv_bwd_f32(d, op.x, op.dy, op.w.reshape(-1), mb, dw, need_dx=True, dx=dx)
      _verify('bwd_f32.dx (no addend) ' + nm, dx, chk, E.f32_pattern(ref['dx']))
    del ref
  torch.cuda.synchronize()
  return fig


SETS = ['small', 'pp', 'stem', 'c3', 'rs', 'bs', 'resnet50', 'mobilenet_v1', 'vgg', 'dw', 'dw128', 'f32', 'wrn', 'mlp', 'odd']


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--set', default='small', choices=SETS)
  ap.add_argument('--batch', type=int, default=128)
  ap.add_argument('--only', type=int, default=-1)
  ap.add_argument('--regimes', default='low,round')
  ap.add_argument('--workspace', default='pool', choices=['pool', 'exact'])
  a = ap.parse_args()
  if a.workspace == 'pool':
    return walk(a)
  from tests import wsguard
  WS.guard, WS.poisons = wsguard.GuardedWorkspace(), wsguard.POISONS
  with wsguard.installed(WS.guard):
    return walk(a)


def walk(a):
  cases, settings = cases_for(a.set, a.batch), settings_for(a.set)
  run = run_depthwise_case if a.set in ('dw', 'dw128') else run_f32_case if a.set == 'f32' else (
      lambda c, seed, regime, st: run_conv_case(c, seed, regime, st, full=a.set in FULL_SETS, ref_forms=a.set in REF_SETS))
  t0, n = time.time(), 0
  cond = {'max_sum_ab': 0.0, 'min_ties': 1.0, 'min_ties_one_way': 1.0}
  for i, c in enumerate(cases):
    if a.only >= 0 and i != a.only:
      continue
    for regime in a.regimes.split(','):
      try:
        fig = run(c, seed_for(a.set, i), regime, settings)
        _ws_check('end of case %d' % i)
      except AssertionError as e:
        print('FAIL case %d %s %s: %s' % (i, c, regime, e), flush=True)
        print(json.dumps({'ok': False, 'set': a.set, 'case': i, 'shape': list(c), 'regime': regime, 'error': str(e)[:600]}))
        return 1
      for key, v in fig.items():
        if key.startswith('sum_ab_'):
          cond['max_sum_ab'] = max(cond['max_sum_ab'], v)
        if key.startswith('ties_'):
          cond['min_ties'] = min(cond['min_ties'], v[0])
          cond['min_ties_one_way'] = min(cond['min_ties_one_way'], v[1], v[2])
      print('ok case %d %s %s %s' % (i, c, regime, json.dumps(fig)), flush=True)
      torch.cuda.empty_cache()
    n += 1
  verdict = {'ok': True, 'set': a.set, 'cases': n, 'regimes': a.regimes.split(','), 'settings': len(settings),
             'checks': Tally.checks, 'refused': Tally.refused, 'diff_bits': 0, 'guards': 'intact', 'unwritten': 0, 'conditions': cond,
             'seconds': round(time.time() - t0, 1)}
  if WS.guard is not None:
    verdict['workspace'] = dict({'mode': 'exact', 'poisons': ['0x%02X' % p for p in WS.poisons], 'guards': 'intact'},
                                **WS.guard.summary())
    print('workspace by form [requests, largest declared bytes, largest high-water mark]: %s' % json.dumps(WS.by_form), flush=True)
  print(json.dumps(verdict))
  return 0


if __name__ == '__main__':
  sys.exit(main())
