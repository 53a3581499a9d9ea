"""K3 (optimizer.hip) at its edges: the momentum / plain-SGD kernel over the (lr, mu, wd, grad_scale, nesterov) grid of
tests/k23_cases.py on inputs with signed zeros at masked-on and masked-off positions, bit for bit against
oracle.masked_grad + momentum_apply / sgd_apply (w, the slot and the bf16 shadow, between guard bands, the _dlr entry point
on the same inputs); the alignment refusals of the four entry points (RIGL_EINVAL, nothing written); Adam on the
signed-zero inputs against the same masked gradient; and the one deliberate deviation from the reference -- a non-finite
gradient at a masked-off position counts as zero."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

import adam_ref as R  # noqa: E402
import k23_cases as K  # noqa: E402
from test_k2_edges_gpu import Dev  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32


def _u32(a):
  return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


def _eq(what, got, ref):
  got, ref = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(ref).reshape(-1)
  bad = np.nonzero(got.view(got.dtype.str.replace('f', 'u')) != ref.view(ref.dtype.str.replace('f', 'u')))[0]
  assert bad.size == 0, '%s: %d/%d differ, first at %s: got %s ref %s' % (what, bad.size, got.size, bad[:6], got[bad[:6]], ref[bad[:6]])


def _sgd_device(w, g, a, mask, shadow, lr=0.1, offsets=None):
  n = w.size
  spec = dict(w=w, g=g)
  if a is not None:
    spec['a'] = a
  if mask is not None:
    spec['bits'] = K.pack_bits(mask)
  if shadow:
    spec['sh'] = np.full(n, 0x4100, np.uint16)
  spec['lr'] = np.full(1, lr, F32)                        # the rate cell of the _dlr entry point
  return Dev(K.Placement(spec, 0, offsets=offsets))


def _step(D, cfg, dlr=False):
  """One update; with `dlr` the rate is the one _sgd_device stored in the rate cell (cfg's is ignored)."""
  from rigl_amd import ops
  lr, mu, wd, gs, nesterov = cfg
  has = D.P.spans
  kw = dict(momentum=D.t('a') if 'a' in has else None, mask_bits=D.t('bits') if 'bits' in has else None, mu=mu, weight_decay=wd,
            grad_scale=gs, nesterov=nesterov, w_shadow=D.t('sh') if 'sh' in has else None)
  if dlr:
    ops.masked_sgd_momentum(D.t('w'), D.t('g'), lr_device=D.t('lr'), **kw)
  else:
    ops.masked_sgd_momentum(D.t('w'), D.t('g'), lr, **kw)


@pytest.mark.parametrize('n', K.SIZES)
def test_momentum_grid_with_signed_zeros(n):
  w, g, a, mask = K.momentum_inputs(n)
  for cfg in K.MOMENTUM_GRID:
    for use_mask in (True, False):
      for has_mom in (True, False):
        w1, a1, sh1 = K.momentum_ref(w, g, a, mask if use_mask else None, *cfg, has_mom=has_mom)
        for shadow in (True, False):
          for dlr in (False, True):
            D = _sgd_device(w, g, a if has_mom else None, mask if use_mask else None, shadow, lr=cfg[0])
            _step(D, cfg, dlr)
            host = D.host()
            what = 'n=%d cfg=%s mask=%d mom=%d shadow=%d dlr=%d' % (n, cfg, use_mask, has_mom, shadow, dlr)
            v = D.P.views(host)
            assert D.P.guards_intact(host), what + ': guard hit'
            _eq(what + ' w', v['w'], w1)
            if has_mom:
              _eq(what + ' slot', v['a'], a1)
            if shadow:
              _eq(what + ' shadow', v['sh'], sh1)
            _eq(what + ' grad (read only)', v['g'], g)


def test_signed_zero_momentum_of_a_pruned_weight_keeps_its_sign():
  """The case of the two yardsticks: a = -0.0, mask off, g < 0, w < 0, wd = 0 -- the reference keeps a = -0.0."""
  n = 64
  w, g, a = np.full(n, -1.5, F32), np.full(n, -2.0, F32), np.full(n, -0.0, F32)
  mask = (np.arange(n) % 2).astype(F32)
  D = _sgd_device(w, g, a, mask, True)
  _step(D, (0.1, 0.9, 0.0, 1.0, True))
  v = D.P.views(D.host())
  w1, a1, sh1 = K.momentum_ref(w, g, a, mask, 0.1, 0.9, 0.0, 1.0, True)
  assert (_u32(a1)[mask == 0] == 0x80000000).all()
  _eq('slot', v['a'], a1)
  _eq('w', v['w'], w1)
  _eq('shadow', v['sh'], sh1)


@pytest.mark.parametrize('gs', [1.0, 0.125])
def test_non_finite_gradient_at_a_masked_off_position_counts_as_zero(gs):
  """The deliberate deviation: the reference's mask * g would put NaN into a pruned weight (0 * inf); here the element is
  a zero with the gradient's sign.  Masked-on elements take the non-finite gradient as it is."""
  n = 4099
  w, g, a, mask = K.momentum_inputs(n)
  k = np.arange(n)
  bad = (k % 9 == 4) & (mask == 0)
  vals = np.array([np.inf, -np.inf], F32) if gs != 1.0 else np.array([np.inf, -np.inf, np.nan, -np.nan], F32)
  g = g.copy()
  g[bad] = vals[k[bad] % vals.size]
  g_as_zero = np.where(bad, np.copysign(F32(0), g), g).astype(F32)
  for cfg in [(0.1, 0.9, 0.0, gs, True), (0.1, 0.9, 1e-4, gs, False)]:
    D = _sgd_device(w, g, a, mask, True)
    _step(D, cfg)
    v = D.P.views(D.host())
    w1, a1, sh1 = K.momentum_ref(w, g_as_zero, a, mask, *cfg)
    assert not np.isnan(w1).any()
    _eq('w %s' % (cfg,), v['w'], w1)
    _eq('slot %s' % (cfg,), v['a'], a1)
    _eq('shadow %s' % (cfg,), v['sh'], sh1)
  # Adam: the same rule
  m0, v0 = (a * F32(0.1)).astype(F32), np.abs(a).astype(F32)
  bp = np.array([F32(0.9) ** 3, F32(0.999) ** 3], F32)
  D = Dev(K.Placement(dict(w=w, g=g, m=m0, v=v0, bits=K.pack_bits(mask), bp=bp)))
  from rigl_amd import ops
  ops.masked_adam(D.t('w'), D.t('g'), D.t('m'), D.t('v'), D.t('bp'), 3e-3, mask_bits=D.t('bits'), grad_scale=gs)
  host = D.host()
  assert D.P.guards_intact(host)
  vv = D.P.views(host)
  w1, m1, v1 = R.adam_apply(w, m0, v0, R.masked_grad(g_as_zero, mask, w, 0.0, gs), 3e-3, bp)
  _eq('adam w', vv['w'], w1)
  _eq('adam m', vv['m'], m1)
  _eq('adam v', vv['v'], v1)


# ---- refusals ---------------------------------------------------------------------------------------------------------
def _refused(call, D, what):
  from rigl_amd import _lib
  before = D.host().copy()
  with pytest.raises(_lib.RiglError) as e:
    call()
  assert e.value.code == _lib.RIGL_EINVAL, what
  assert np.array_equal(D.host(), before), what + ': something was written'


@pytest.mark.parametrize('n', [5, 4097])
def test_misaligned_operands_are_refused_with_nothing_written(n):
  from rigl_amd import ops
  w, g, a, mask = K.momentum_inputs(n)
  v0 = np.abs(a)
  bp = np.array([0.9, 0.999], F32)
  for name in ('w', 'g', 'a', 'sh'):
    for off in (1, 2, 3):                   # fp32: 4, 8, 12 bytes off a 16-byte boundary; bf16: 2, 4, 6 bytes off an 8-byte one
      what = '%s off %d' % (name, off)
      D = _sgd_device(w, g, a, mask, True, offsets={name: off})
      _refused(lambda: _step(D, (0.1, 0.9, 1e-4, 1.0, True)), D, 'momentum ' + what)
      _refused(lambda: _step(D, (0.1, 0.9, 1e-4, 1.0, True), dlr=True), D, 'momentum dlr ' + what)
  for name in ('w', 'g', 'm', 'v', 'sh'):
    for off in (1, 2, 3):
      what = '%s off %d' % (name, off)
      D = Dev(K.Placement(dict(w=w, g=g, m=a, v=v0, bits=K.pack_bits(mask), sh=np.full(n, 0x4100, np.uint16), bp=bp, lr=np.full(1, 3e-3, F32)),
                          0, offsets={name: off}))
      kw = dict(mask_bits=D.t('bits'), weight_decay=1e-4, w_shadow=D.t('sh'))
      _refused(lambda: ops.masked_adam(D.t('w'), D.t('g'), D.t('m'), D.t('v'), D.t('bp'), 3e-3, **kw), D, 'adam ' + what)
      _refused(lambda: ops.masked_adam(D.t('w'), D.t('g'), D.t('m'), D.t('v'), D.t('bp'), lr_device=D.t('lr'), **kw), D,
               'adam dlr ' + what)


# ---- Adam on the signed zeros -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [5, 1025, 4097])
def test_adam_on_signed_zeros_against_the_unified_masked_gradient(n):
  from rigl_amd import ops
  w, g, m0, mask = K.momentum_inputs(n)
  m0 = np.where(np.abs(m0) > 1e20, F32(0.5), m0).astype(F32)
  v0 = np.where(np.arange(n) % 4 == 0, 0, np.abs(m0)).astype(F32)
  bp = np.array([F32(0.9) ** 3, F32(0.999) ** 3], F32)
  for use_mask in (True, False):
    for wd, gs in ((0.0, 1.0), (1e-4, 0.125), (0.0, 0.125), (1e-4, 1.0)):
      for dlr in (False, True):
        spec = dict(w=w, g=g, m=m0, v=v0, sh=np.full(n, 0x4100, np.uint16), bp=bp, lr=np.full(1, 3e-3, F32))
        if use_mask:
          spec['bits'] = K.pack_bits(mask)
        D = Dev(K.Placement(spec))
        rate = dict(lr_device=D.t('lr')) if dlr else dict(lr=float(F32(3e-3)))
        ops.masked_adam(D.t('w'), D.t('g'), D.t('m'), D.t('v'), D.t('bp'), mask_bits=D.t('bits') if use_mask else None, weight_decay=wd,
                        grad_scale=gs, w_shadow=D.t('sh'), **rate)
        host = D.host()
        what = 'n=%d mask=%d wd=%g gs=%g dlr=%d' % (n, use_mask, wd, gs, dlr)
        assert D.P.guards_intact(host), what
        v = D.P.views(host)
        with np.errstate(all='ignore'):
          w1, m1, v1 = R.adam_apply(w, m0, v0, R.masked_grad(g, mask if use_mask else None, w, wd, gs), float(F32(3e-3)), bp)
        assert not np.isnan(w1).any()
        _eq(what + ' w', v['w'], w1)
        _eq(what + ' m', v['m'], m1)
        _eq(what + ' v', v['v'], v1)
        sh = K.bf16_bits(w1)
        _eq(what + ' shadow', v['sh'], np.where(mask != 0, sh, 0).astype(np.uint16) if use_mask else sh)
