"""rigl_masked_conv2d_bwd_bnapply: the backward of a 1x1 / 64 -> 256 conv that applies the backward of the batch norm BEHIND it
(bn3 of a bottleneck block: relu(bn3(conv3) + shortcut)) on its own dY load (bwd1x1.hpp, BNA), after rigl_bn_bwd_reduce.

Held two ways:
* bit for bit (raw bf16 / fp32 patterns) against the pair of calls it replaces, rigl_bn_bwd followed by rigl_masked_conv2d_bwd
  on the same single-pass kernel: dX, dW, dgamma, dbeta;
* to float64 through the project's references, link by link: the gradient the batch norm hands to the conv (rigl_bn_bwd's dx,
  which the fused kernel forms in LDS -- the bit-equality above is what ties the two) to tests/bn_ref.py's check_backward, and
  the fused call's dX / dW to tests/convref.py's conv_fp64 fed that bf16 tensor, the operand the kernel multiplies (convref's
  convention: "the SAME bf16-rounded values the kernels read"), inside its bound 2^-8 |ref| + 1e-5 sum |a| |b| (dW: no output
  rounding).

Shapes: M = 3 x 53 x 53 = 8 427 rows is the smallest of this family the body takes (knob "bwd1x1" = 2: from 8 192 rows): 264
K-tiles of 32 rows for 2 x CUs workgroups, so workgroups own zero tiles and the last tile has 11 rows; and M = 4 x 56 x 56.
Each with and without an addend on dX, gamma normal / negative / all-zero (bn3 starts at zero in ResNet-50: dy3 is +-0 and the
zero's sign must survive), random ReLU bits with one all-off and one all-on row.  Every case prints its worst ratios.
"""
import pytest

torch = pytest.importorskip('torch')

from tests import bn_ref as R  # noqa: E402
from tests import convref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CI, CO = 64, 256
SHAPES = ((3, 53, 53), (4, 56, 56))
GAMMAS = ('normal', 'negative', 'zero')
EPS = 1e-5


@pytest.fixture(scope='module', autouse=True)
def _knobs():
  from rigl_amd import ops
  ops.tune_set('bwd1x1', 2)
  ops.tune_set('bn_bwd_on_load', 1)
  yield
  ops.tune_unset('bwd1x1')
  ops.tune_unset('bn_bwd_on_load')


_CACHE = {}


def _inputs(shape):
  """The operands of one shape, made once: x, the packed weight, y3 = conv(x), dout, the addend, the ReLU bits."""
  if shape in _CACHE:
    return _CACHE[shape]
  from rigl_amd import ops
  n, h, w = shape
  m = n * h * w
  gen = torch.Generator(device='cpu').manual_seed(7 + m)
  d = ops.conv_desc(n, h, w, CI, CO, 1, 1, 1, 0, 0, h, w)
  x = (torch.randn(n, h, w, CI, generator=gen) * 0.5).to(torch.bfloat16).to(DEV)
  wf = (torch.randn(CI * CO, generator=gen) * (2.0 / CI) ** 0.5).to(DEV)
  hwio = torch.empty(CI * CO, dtype=torch.bfloat16, device=DEV)
  ohwi = torch.empty(CI * CO, dtype=torch.bfloat16, device=DEV)
  ops.pack_weights(wf, None, CI, CO, hwio, ohwi)
  y3 = ops.conv_fwd(d, x, ohwi).reshape(m, CO)
  dout = torch.randn(m, CO, generator=gen).to(torch.bfloat16).to(DEV)
  addend = torch.randn(n, h, w, CI, generator=gen).to(torch.bfloat16).to(DEV)
  on = torch.rand(m, CO, generator=gen) < 0.5
  on[0] = False            # an all-off row
  on[1] = True             # an all-on row
  on[m - 1, ::2] = True    # (and the very last row, in the ragged tile, is not trivially empty)
  bits = R.pack_bits(on).to(DEV)
  st = R.stats_ref(y3, EPS)
  _CACHE[shape] = dict(d=d, x=x, hwio=hwio, y3=y3, dout=dout, addend=addend, on=on.to(DEV), bits=bits, st=st, m=m)
  return _CACHE[shape]


def _gamma(kind):
  gen = torch.Generator(device='cpu').manual_seed(11)
  g = torch.randn(CO, generator=gen)
  if kind == 'negative':
    g = -g.abs() - 0.125
  if kind == 'zero':
    g = torch.zeros(CO)
  return g.to(DEV)


def _b16(t):
  return t.contiguous().view(torch.int16)


def _b32(t):
  return t.contiguous().view(torch.int32)


@pytest.mark.parametrize('gamma_kind', GAMMAS)
@pytest.mark.parametrize('with_addend', (False, True), ids=('plain', 'addend'))
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_fused_backward_equals_the_two_calls_and_fp64(shape, with_addend, gamma_kind):
  from rigl_amd import ops
  I = _inputs(shape)
  d, x, hwio, y3, dout, bits, m = I['d'], I['x'], I['hwio'], I['y3'], I['dout'], I['bits'], I['m']
  name = '%s %s gamma=%s' % ('x'.join(map(str, shape)), 'addend' if with_addend else 'plain', gamma_kind)
  assert ops.conv_bwd_takes_bn_apply(d), name + ': the layer must take the transform at this size'
  gamma, beta = _gamma(gamma_kind), torch.zeros(CO, device=DEV)
  rm, rv = torch.zeros(CO, device=DEV), torch.ones(CO, device=DEV)
  saved = ops.bn_fwd(y3, gamma, beta, rm, rv, 0.1, EPS, True, None)[1]       # (mean, invstd, scale, shift of y3)
  addend = I['addend'] if with_addend else None
  # ---- the two calls -----------------------------------------------------------------------------------------------
  dg0, db0 = torch.full((CO,), 7.0, device=DEV), torch.full((CO,), 7.0, device=DEV)
  dy3, _ = ops.bn_bwd(y3, None, dout, gamma, saved, True, dg0, db0, want_dres=False, relu_bits=bits)
  dw0 = torch.full((CI * CO,), 7.0, device=DEV)
  dx0 = ops.conv_bwd(d, x, dy3.reshape(d.n, d.h, d.w, CO), hwio, dw0, need_dx=True, addend=addend)
  # ---- the fused pair ----------------------------------------------------------------------------------------------
  dg1, db1 = torch.full((CO,), -7.0, device=DEV), torch.full((CO,), -7.0, device=DEV)
  coef = ops.bn_bwd_reduce(y3, dout, gamma, saved, True, bits, dg1, db1)
  dw1 = torch.full((CI * CO,), -7.0, device=DEV)
  dx1 = ops.conv_bwd_bnapply(d, x, dout, hwio, dw1, y3, bits, saved, coef, addend=addend)
  torch.cuda.synchronize()
  assert torch.equal(_b32(dg1), _b32(dg0)), name + ': dgamma differs from rigl_bn_bwd\'s in bits'
  assert torch.equal(_b32(db1), _b32(db0)), name + ': dbeta differs from rigl_bn_bwd\'s in bits'
  bad = (_b16(dx1) != _b16(dx0))
  assert not bool(bad.any()), '%s: dX differs in bits at %d elements, first flat index %d' % (
      name, int(bad.sum()), int(bad.reshape(-1).nonzero()[0]))
  bad = (_b32(dw1) != _b32(dw0))
  assert not bool(bad.any()), '%s: dW differs in bits at %d elements, first flat index %d' % (
      name, int(bad.sum()), int(bad.reshape(-1).nonzero()[0]))
  # ---- float64, link by link ---------------------------------------------------------------------------------------
  worst = R.check_backward(name, y3, dout, I['on'], gamma, I['st'], dy3, dg1, db1)
  w4 = hwio.reshape(1, 1, CI, CO)
  dy4 = dy3.reshape(d.n, d.h, d.w, CO)
  ref = convref.conv_fp64(x, w4, dy4, 1, 0, 0, d.h, d.w, want=('dx', 'dw'))
  mag = convref.conv_fp64(x.abs(), w4.abs(), dy4.abs(), 1, 0, 0, d.h, d.w, want=('dx', 'dw'))
  dx_ref, dx_mag = ref['dx'], mag['dx']
  if with_addend:
    # bf16(bf16(dgrad) + addend): the inner rounding is one more 2^-8 of the dgrad, carried in the magnitude term
    # (times 1 + 2^-7: the outer rounding acts on the computed sum, which carries the inner error)
    dx_mag = dx_mag * (1 + 2.0**-7) + 2.0**-8 * (1 + 2.0**-7) / 1e-5 * dx_ref.abs() + addend.double().abs()
    dx_ref = dx_ref + addend.double()
  worst['dX'] = convref.check_close(name + ' dX', dx1, dx_ref, dx_mag, out_ulp=2.0**-8)
  worst['dW'] = convref.check_close(name + ' dW', dw1.reshape(1, 1, CI, CO), ref['dw'], mag['dw'])
  if gamma_kind == 'zero':
    assert bool((dw1 == 0).all()), name + ': dW is not zero although every dy3 is'
  print('%s: worst ratios %s' % (name, {k: round(float(v), 4) for k, v in worst.items()}))


def test_the_transform_is_refused_where_the_layer_does_not_take_it():
  """The query and the entry point agree: another channel count, or the knob off, is RIGL_EUNSUPPORTED, never a silent
  fall-back to another kernel."""
  from rigl_amd import ops
  I = _inputs(SHAPES[0])
  d64 = ops.conv_desc(3, 53, 53, 64, 64, 1, 1, 1, 0, 0, 53, 53)
  assert not ops.conv_bwd_takes_bn_apply(d64)
  ops.tune_set('bn_bwd_on_load', 0)
  try:
    assert not ops.conv_bwd_takes_bn_apply(I['d'])
    with pytest.raises(ValueError):
      ops.conv_bwd_bnapply(I['d'], I['x'], I['dout'], I['hwio'], torch.empty(CI * CO, device=DEV), I['y3'], I['bits'],
                           torch.zeros(4, CO, device=DEV), torch.zeros(3, CO, device=DEV))
  finally:
    ops.tune_set('bn_bwd_on_load', 1)
