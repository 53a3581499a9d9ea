"""The direct conv kernels (rigl_conv2d_{fwd,dgrad,wgrad}_ref, conv_ref.hip) validate their descriptors like every other K1
entry point: a zero or negative dimension and an output grid one row larger than input / stride / pad allow are RIGL_EINVAL, a
tensor of 2^30 elements by the descriptor's own arithmetic is RIGL_EUNSUPPORTED -- before a pointer is used, with nothing
launched: the guarded outputs are all sentinel afterwards -- and the valid neighbours of the bad descriptors still run and give
the exact bits (tests/exactref.py).

Every buffer of a refusal that could launch is sized by the descriptor's own claims, so a MISSING refusal would write inside
the test's allocation; the 2^30-element descriptors are refused from their arithmetic alone (their tensors are never made)."""
import ctypes as C

import pytest
import torch

from tests import exactref as E

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF, F32 = torch.bfloat16, torch.float32

# N, H, W, Cin, Cout, k, stride, pad_top, pad_left, Ho, Wo: neither channel count a multiple of 8 (ordinary dispatch goes to
# the direct kernels), a 3x3 with padding 1
BASE = (2, 6, 7, 5, 6, 3, 1, 1, 1, 6, 7)
# Ho = 7: the windows of the last output row start in the bottom padding row -- the largest grid check_desc admits; Ho = 8 is
# one more than input / stride / pad allow
TALL = BASE[:9] + (7, 7)

BAD = [
    ('n = 0', dict(n=0), 'EINVAL'), ('cin = 0', dict(cin=0), 'EINVAL'), ('cout = 0', dict(cout=0), 'EINVAL'),
    ('h = 0', dict(h=0), 'EINVAL'), ('wo = 0', dict(wo=0), 'EINVAL'), ('kw = 0', dict(kw=0), 'EINVAL'),
    ('n = -1', dict(n=-1), 'EINVAL'), ('cin = -5', dict(cin=-5), 'EINVAL'), ('kh = -3', dict(kh=-3), 'EINVAL'),
    ('stride_h = -1', dict(stride_h=-1), 'EINVAL'), ('pad_left = -1', dict(pad_left=-1), 'EINVAL'),
    ('ho = 8 (one more than the input allows)', dict(ho=8), 'EINVAL'),
    ('wo = 9 (one more than the input allows)', dict(wo=9), 'EINVAL'),
]
# x and y of 2^30 elements (the limit is 2^30 - 1); w of 2^30 elements behind a one-pixel image
HUGE = [
    ('x, y of 2^30 elements', dict(n=1 << 15, h=1 << 15, w=1, cin=1, cout=1, kh=1, kw=1, stride_h=1, stride_w=1, pad_top=0,
                                   pad_left=0, ho=1 << 15, wo=1)),
    ('w of 2^30 elements', dict(n=1, h=1, w=1, cin=1 << 15, cout=1 << 15, kh=1, kw=1, stride_h=1, stride_w=1, pad_top=0,
                                pad_left=0, ho=1, wo=1)),
]


def _desc(case, **over):
  from rigl_amd import ops
  N, H, W, Cin, Cout, k, stride, pt, pl, Ho, Wo = case
  d = ops.conv_desc(N, H, W, Cin, Cout, k, k, stride, pt, pl, Ho, Wo)
  for key, v in over.items():
    setattr(d, key, v)
  return d


def _claims(d):
  """Element counts of x, w, y by the descriptor's own arithmetic, at least one each."""
  return (max(1, d.n * d.h * d.w * d.cin), max(1, d.kh * d.kw * d.cin * d.cout), max(1, d.n * d.ho * d.wo * d.cout))


def _sentinel_only(name, buf):
  sent = E.SENTINEL16 if buf.dtype == torch.int16 else E.SENTINEL32
  assert bool((buf == sent).all()), '%s: refused, yet an output buffer was written' % name


def _call_all(d, nx, nw, ny):
  """The three entry points on zero-filled operands of the given sizes and guarded outputs: [(name, code, output buffer)]."""
  from rigl_amd import _lib
  lib = _lib.load()
  x, w, dy = (torch.zeros(n, dtype=BF, device=DEV) for n in (nx, nw, ny))
  out = []
  for name, fn, a, b, shape, dtype in (('fwd_ref', lib.rigl_conv2d_fwd_ref, x, w, (ny,), BF),
                                       ('dgrad_ref', lib.rigl_conv2d_dgrad_ref, dy, w, (nx,), BF),
                                       ('wgrad_ref', lib.rigl_conv2d_wgrad_ref, x, dy, (nw,), F32)):
    o, _, buf = E.guarded(shape, dtype, DEV)
    rc = fn(C.byref(d), a.data_ptr(), b.data_ptr(), o.data_ptr(), None)
    torch.cuda.synchronize()
    out.append((name, rc, buf))
  return out


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')
@pytest.mark.parametrize('what,over,code', BAD, ids=[b[0].split(' (')[0] for b in BAD])
def test_bad_descriptors_are_refused_with_nothing_written(what, over, code):
  from rigl_amd import _lib
  d = _desc(BASE, **over)
  for name, rc, buf in _call_all(d, *_claims(d)):
    assert rc == getattr(_lib, 'RIGL_' + code), '%s, %s: returned %d, RIGL_%s expected' % (what, name, rc, code)
    _sentinel_only('%s, %s' % (what, name), buf)


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')
@pytest.mark.parametrize('what,fields', HUGE, ids=['activations', 'weights'])
def test_a_tensor_of_2_to_the_30_elements_is_unsupported(what, fields):
  from rigl_amd import _lib
  d = _desc(BASE, **fields)
  assert max(d.n * d.h * d.w * d.cin, d.kh * d.kw * d.cin * d.cout, d.n * d.ho * d.wo * d.cout) == 1 << 30
  for name, rc, buf in _call_all(d, 64, 64, 64):
    assert rc == _lib.RIGL_EUNSUPPORTED, '%s, %s: returned %d, RIGL_EUNSUPPORTED expected' % (what, name, rc)
    _sentinel_only('%s, %s' % (what, name), buf)


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')
@pytest.mark.parametrize('case', [BASE, TALL], ids=['base', 'tallest-grid'])
@pytest.mark.parametrize('regime', ['low', 'round'])
def test_the_valid_neighbours_run_and_give_the_exact_bits(case, regime):
  """The descriptor every bad one above was made from, and the tallest output grid check_desc admits (one row fewer than the
  refused one): through ordinary dispatch (cout % 8 != 0: the direct kernels), bit for bit, guards intact, nothing unwritten."""
  from rigl_amd import ops
  N, H, W, Cin, Cout, k, stride, pt, pl, Ho, Wo = case
  op = E.operands(case, 101, regime, DEV)
  ref, ab = E.reference(op)
  for key, unit in (('y', op.uy), ('dx', op.udx), ('dw', op.udw)):
    assert float(ab[key].max()) / unit <= E.LIMIT
  d = _desc(case)
  assert not ops.mfma_supported(d)
  x, dy = op.x.to(BF), op.dy.to(BF)
  wm = op.wm.to(BF)
  hwio = wm.reshape(-1).contiguous()
  ohwi = wm.reshape(k * k * Cin, Cout).t().contiguous().reshape(-1)
  y, chk, _ = E.guarded((N, Ho, Wo, Cout), BF, DEV)
  ops.conv_fwd(d, x, ohwi, y=y)
  chk('fwd')
  E.assert_bits('fwd', E.got_bits(y), E.expect_plain(ref['y']))
  dx, chk, _ = E.guarded((N, H, W, Cin), BF, DEV)
  ops.conv_dgrad(d, dy, hwio, dx=dx)
  chk('dgrad')
  E.assert_bits('dgrad', E.got_bits(dx), E.expect_plain(ref['dx']))
  dw, chk, _ = E.guarded((k * k * Cin * Cout,), F32, DEV)
  ops.conv_wgrad(d, x, dy, dw=dw)
  chk('wgrad')
  E.assert_bits('wgrad', E.got_bits(dw), E.f32_pattern(ref['dw'].reshape(-1)))
