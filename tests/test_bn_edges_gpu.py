"""The batch-norm kernels (rigl_amd/csrc/bn.hip) held to the float64 references of tests/bn_ref.py at the eight ResNet-50
batch-norm tensors of batch 128, at the small shapes where the row partition is ragged, and on data a sparse network
produces: all-zero and constant channels, channels far from zero, tiny and large ones, post-ReLU inputs, gamma = 0.

Nothing compared against touches the library: the references run in this process in float64 (on the device for the
large tensors, in row chunks).  The saved scale / shift rows are held to the float64 statistics, and the apply pass to its
exact restatement fed those rows, bit for bit with no element excluded.  Every bound is one of bn_ref's, and
tests/test_bn_ref_cpu.py shows an fp32 restatement of the kernels inside half of each on the same small inputs.  Every
test prints its worst figures before it returns.

Wall time on an MI355X, one pytest process each: this file 7.7 s (45 tests; 9 s with start-up), the parent commit's
tests/test_bn_gpu.py 3.8 s -- the float64 references of the batch-128 tensors run on the device.
"""
import pytest

torch = pytest.importorskip('torch')

from tests import bn_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _ids(s):
  return 'x'.join(map(str, s))


def _rows(shape):
  return shape[0] * shape[1] * shape[2], shape[3]


def _inputs(shape, seed=1):
  """edge_tensor as [M, C] on the device; the small shapes are generated on the CPU, so they are the very tensors of
  tests/test_bn_ref_cpu.py."""
  m, c = _rows(shape)
  dev = 'cpu' if m * c <= (1 << 24) else DEV
  return tuple(t.to(DEV) for t in R.edge_tensor(m, c, seed, device=dev))


def _b16(t):
  return t.contiguous().view(torch.int16)


def _fold(worst, w):
  for k, v in w.items():
    worst[k] = max(worst.get(k, 0), v)


def _forward(name, x, res, gamma, beta, eps, momentum, relu, worst, partials=None, st=None):
  """One forward held to every check of the issue; -> (y, saved, bits, statistics)."""
  from rigl_amd import ops
  c = x.shape[1]
  rm0, rv0 = (t.to(DEV) for t in R.moving_start(c, 1))
  rm, rv = rm0.clone(), rv0.clone()
  out = ops.bn_fwd(x, gamma, beta, rm, rv, momentum, eps, relu, res, partials=partials, want_relu_bits=relu)
  y, saved, bits = out[0], out[1], (out[2] if relu else None)
  st = st or R.stats_ref(x, eps)
  R.check_statistics(name, st, gamma, beta, saved, rm0, rv0, rm, rv, momentum, worst=worst)
  ye, be = R.apply_exact(x, saved[2], saved[3], relu, res)
  assert torch.equal(_b16(y), _b16(ye)), name + ': y is not the exact apply stage of the saved scale / shift'
  if relu:
    assert torch.equal(bits, be), name + ': the ReLU bits are not those of the exact apply stage'
  del ye, be
  R.check_forward(name, x, res, gamma, beta, st, relu, y, bits, worst=worst)
  zc = R.zero_channels(x)
  if bool(zc.any()):
    assert bool((saved[1][zc] == R.invstd_of_zero_variance(eps).to(DEV)).all()), name + ': invstd of an all-zero channel'
    v = beta[zc].expand(x.shape[0], -1)
    if res is not None:
      v = v + res[:, zc].float()
    if relu:
      v = v.clamp_min(0)
    assert torch.equal(y[:, zc], v.to(torch.bfloat16)), name + ': y of an all-zero channel is not bf16(beta (+ res))'
  return y, saved, bits, st


def _backward(name, x, dy, y, bits, gamma, saved, st, relu, with_res, worst):
  """The backward with the mask the forward left, held to the references, and the three mask sources against each other."""
  from rigl_amd import ops
  c = x.shape[1]
  on = R.unpack_bits(bits, x.shape) if relu else None
  dg, db = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
  dx, dres = ops.bn_bwd(x, None, dy, gamma, saved, relu, dg, db, want_dres=with_res, relu_bits=bits)
  R.check_backward(name, x, dy, on, gamma, st, dx, dg, db, dres, worst=worst)
  del on
  if relu:
    sources = [('saved y', dict(y=y))] + ([] if with_res else [('recomputed', dict(y=None))])
    for what, kw in sources:
      dg1, db1 = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
      dx1, dres1 = ops.bn_bwd(x, kw['y'], dy, gamma, saved, relu, dg1, db1, want_dres=with_res)
      assert torch.equal(_b16(dx), _b16(dx1)) and torch.equal(dg, dg1) and torch.equal(db, db1), \
          '%s: the %s mask does not give the bits of the 1-bit mask' % (name, what)
      if with_res:
        assert torch.equal(_b16(dres), _b16(dres1))
  return dx, dg, db


def _sweep(shape, backward=True, combos=R.RELU_RES, settings=R.EPS_MOMENTUM):
  x, dy, res, gamma, beta = _inputs(shape)
  worst = {}
  for eps, momentum in settings:
    st = R.stats_ref(x, eps)
    for relu, with_res in combos:
      name = '%s eps=%g relu=%d res=%d' % (_ids(shape), eps, relu, with_res)
      rr = res if with_res else None
      y, saved, bits, _ = _forward(name, x, rr, gamma, beta, eps, momentum, relu, worst, st=st)
      if backward:
        _backward(name, x, dy, y, bits, gamma, saved, st, relu, with_res, worst)
  return worst


def _show(what, worst):
  print('%s: worst error / bound %s' % (what, {k: float('%.3g' % v) for k, v in worst.items()}))


@pytest.mark.parametrize('shape', R.RESNET50_BN + R.SMALL_SHAPES + R.CAP_SHAPES, ids=_ids)
def test_forward_and_backward_on_edge_tensor(shape):
  """All four (relu, residual) combinations x both (eps, momentum) settings, non-trivial initial moving averages."""
  _show(_ids(shape), _sweep(shape))


def test_4096_channels_forward_and_the_backward_refusal():
  """C = 4096: two blockIdx.y slabs of k_reduce with one row per pass.  The backward stages 7 * C floats in LDS and
  refuses the layer; that refusal has to be the clean RIGL_EUNSUPPORTED."""
  from rigl_amd import _lib, ops
  _show(_ids(R.WIDE_SHAPE), _sweep(R.WIDE_SHAPE, backward=False))
  x, dy, res, gamma, beta = _inputs(R.WIDE_SHAPE)
  y, saved = ops.bn_fwd(x, gamma, beta, None, None, 0.1, 1e-5, False)
  dg, db = torch.empty(4096, device=DEV), torch.empty(4096, device=DEV)
  with pytest.raises(_lib.RiglError) as ei:
    ops.bn_bwd(x, None, dy, gamma, saved, False, dg, db)
  assert ei.value.code == _lib.RIGL_EUNSUPPORTED


KNOB_SHAPES = R.SMALL_SHAPES + R.CAP_SHAPES + ((128, 56, 56, 64), (128, 14, 14, 1024))


@pytest.mark.parametrize('shape', KNOB_SHAPES, ids=_ids)
@pytest.mark.parametrize('knob', ['bn_il', 'bn_regs'])
def test_layout_and_staging_knobs(knob, shape):
  """The contiguous row partition ("bn_il" = 0) and the LDS parameter staging ("bn_regs" = 0) under the same checks."""
  from rigl_amd import ops
  ops.tune_set(knob, 0)
  try:
    worst = _sweep(shape, settings=R.EPS_MOMENTUM[:1] if shape[0] == 128 else R.EPS_MOMENTUM)
  finally:
    ops.tune_unset(knob)
  _show('%s=0 %s' % (knob, _ids(shape)), worst)


@pytest.mark.parametrize('shape', [(128, 56, 56, 64), (128, 112, 112, 64)], ids=_ids)
def test_producer_partials_through_the_one_channel_finalize(shape):
  """bn_fwd fed 128-row partial sums (sum x, sum x^2 in float64, rounded to fp32) as a conv epilogue leaves them: 3 136
  and 12 544 of them, both above the 1 024 at which k_fwd_finalize<1> takes over.  Same bounds as the self-reducing
  forward; the apply pass stays bit-exact."""
  m, c = _rows(shape)
  x, _, res, gamma, beta = _inputs(shape)
  parts = m // 128
  assert parts * 128 == m and parts > 1024
  partials = torch.empty(parts, 2, c, dtype=torch.float32, device=DEV)
  step = 1024
  for p0 in range(0, parts, step):
    xd = x[p0 * 128:(p0 + step) * 128].double().reshape(-1, 128, c)
    partials[p0:p0 + step, 0] = xd.sum(1).float()
    partials[p0:p0 + step, 1] = (xd * xd).sum(1).float()
  worst = {}
  for (eps, momentum), (relu, with_res) in zip(R.EPS_MOMENTUM, ((True, True), (False, False))):
    _forward('%s from %d partials' % (_ids(shape), parts), x, res if with_res else None, gamma, beta, eps, momentum,
             relu, worst, partials=partials)
  _show('%s from %d partials' % (_ids(shape), parts), worst)


@pytest.mark.parametrize('shape', R.SMALL_SHAPES + ((128, 28, 28, 128), (128, 7, 7, 2048)), ids=_ids)
def test_frozen_apply_is_the_exact_apply_stage(shape):
  """ops.bn_apply / ops.bn_apply_pair (the eval path) with arbitrary scale / shift -- zero, negative, 2^-10 and large
  scales among them -- bit-identical to the exact apply stage."""
  from rigl_amd import ops
  x, x2, res, gamma, beta = _inputs(shape)
  c = x.shape[1]
  g = torch.Generator().manual_seed(c)
  ss = torch.stack([gamma * 3.0, beta]).contiguous()
  ss2 = torch.stack([torch.randn(c, generator=g).to(DEV) * 0.01, gamma]).contiguous()
  for relu in (False, True):
    for rr in (None, res):
      y = ops.bn_apply(x, ss, relu=relu, residual=rr)
      assert torch.equal(_b16(y), _b16(R.apply_exact(x, ss[0], ss[1], relu, rr)[0])), (shape, relu, rr is not None)
    y = ops.bn_apply_pair(x, x2, ss, ss2, relu=relu)
    short = R.apply_exact(x2, ss2[0], ss2[1], False)[0]              # the shortcut as its own batch norm would store it
    assert torch.equal(_b16(y), _b16(R.apply_exact(x, ss[0], ss[1], relu, short)[0])), (shape, relu, 'pair')


@pytest.mark.parametrize('shape', [(33, 3, 3, 40), (128, 28, 28, 128)], ids=_ids)
def test_an_overflowing_channel_leaves_the_others_alone(shape):
  """One channel of x is 3e38 everywhere (its x^2 overflows fp32); every other channel's saved statistics, moving
  averages, y, dx, dres, dgamma and dbeta keep the bits of the clean run.  Ordinary buffers throughout."""
  from rigl_amd import ops
  x, dy, res, gamma, beta = _inputs(shape)
  c = x.shape[1]
  bad = 13
  keep = torch.arange(c, device=DEV) != bad
  outs = []
  for poison in (False, True):
    xx = x.clone()
    if poison:
      xx[:, bad] = 3e38
    rm, rv = (t.to(DEV) for t in R.moving_start(c, 1))
    y, saved, bits = ops.bn_fwd(xx, gamma, beta, rm, rv, 0.1, 1e-5, True, res, want_relu_bits=True)
    dg, db = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
    dx, dres = ops.bn_bwd(xx, None, dy, gamma, saved, True, dg, db, want_dres=True, relu_bits=bits)
    outs.append([saved[:, keep], rm[keep], rv[keep], _b16(y[:, keep]), _b16(dx[:, keep]), _b16(dres[:, keep]), dg[keep],
                 db[keep]])
  for what, a, b in zip(('saved', 'moving mean', 'moving variance', 'y', 'dx', 'dres', 'dgamma', 'dbeta'), *outs):
    assert torch.equal(a, b), '%s of a clean channel changed' % what
    assert not bool(torch.isnan(a.float()).any())


