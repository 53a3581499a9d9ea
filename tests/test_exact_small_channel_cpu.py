"""The small-channel case sets of tests/k1_exact.py (wrn, mlp, odd: k1_check.WRN_CASES / MLP_CASES / ODD_CASES) checked without
a GPU: the input conditions of both regimes at the runner's seeds with y, dx and dw, the plan's worst case from the shape alone,
the runner's own expectation builder on CPU operands, MUTANTS of the direct kernels and of the host fallbacks -- each rejected
by the bit comparison on these sets and, the first four, out of reach of the older `small` set -- and a DRIFT check: the sets
hold the layer shapes of the workloads they stand for, read from the workloads themselves."""
import functools

import pytest
import torch

from tests import exactref as E
from tests import k1_check
from tests import k1_exact

SETS = {'wrn': k1_check.WRN_CASES, 'mlp': k1_check.MLP_CASES, 'odd': k1_check.ODD_CASES}
REGIMES = ('low', 'round')


def test_the_sets_are_the_ones_the_runner_walks():
  assert [len(SETS[s]) for s in ('wrn', 'mlp', 'odd')] == [10, 6, 10]
  for name, cases in SETS.items():
    assert k1_exact.cases_for(name, 128) is cases and name in k1_exact.FULL_SETS and name in k1_exact.REF_SETS
  assert 'small' in k1_exact.REF_SETS and 'small' not in k1_exact.FULL_SETS
  assert k1_exact.settings_for('wrn') == [{}, k1_exact.GENERIC] == k1_exact.settings_for('odd')
  assert k1_exact.settings_for('mlp') == [{}]


@functools.lru_cache(maxsize=None)
def _case(name, i, regime):
  """(op, ref, fig) of case i of a set at the runner's seed: the reference is made once and shared (left unchanged)."""
  op = E.operands(SETS[name][i], k1_exact.seed_for(name, i), regime)
  ref, ab = E.reference(op)
  fig = E.check_conditions(op, ref, ab)
  return op, ref, fig


# ---- conditions -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('name', list(SETS))
def test_input_conditions_with_dx_for_every_case(name, regime):
  """check_conditions asserts them (integers, sum|a||b| <= 2^24 for y, dx AND dw, the 'low' bounds, the 'round' tie shares of y
  and dx) -- dX included for the cin % 8 != 0 shapes, which the older sets never asked for; every operand exact in bf16; and the
  runner's expectation builder (the BN-on-load operand's own sum|a||w| bound) goes through on the same operands."""
  for i, c in enumerate(SETS[name]):
    op, ref, fig = _case(name, i, regime)
    for t in (op.x, op.dy, op.wm, op.add):
      assert torch.equal(t.to(torch.bfloat16).float(), t)
    assert (op.m01 is not None) == (op.seed % 2 == 1)
    assert {'sum_ab_y', 'sum_ab_dx', 'sum_ab_dw'} <= set(fig)
    if regime == 'round':
      assert 'ties_y' in fig and 'ties_dx' in fig
    e = k1_exact.expectations(E.operands(c, op.seed, regime), ref, True)
    assert e.has_dx and e.fused and e.want_dx.shape == op.x.shape


@pytest.mark.parametrize('regime', REGIMES)
def test_plans_keep_the_sums_exact_from_the_shape_alone(regime):
  for name, cases in SETS.items():
    for i, c in enumerate(cases):
      p = E.plan(c, regime, k1_exact.seed_for(name, i) % 2 == 1)
      wc = E.worst_case(c, p)
      assert max(wc.values()) <= E.LIMIT, (name, c, p, wc)
      assert p['ax'] <= 3 and p['ad'] <= 3 and p['aw'] <= 255


# ---- mutants --------------------------------------------------------------------------------------------------------------
def _conv(op, x=None, wm=None, dy=None, want=('y',)):
  N, H, W, Cin, Cout, k, stride, pt, pl, Ho, Wo = op.case
  from tests import convref
  return convref.conv_fp64(op.x if x is None else x, op.wm if wm is None else wm, op.dy if dy is None else dy,
                           stride, pt, pl, Ho, Wo, want)


def _m_cin_tail(op, ref):
  """A direct forward whose channel loop runs in whole groups of 8: the last cin % 8 channels of every tap are left out."""
  c8 = op.case[3] - op.case[3] % 8
  if c8 == op.case[3]:
    return None
  x, wm = op.x.clone(), op.wm.clone()
  x[..., c8:] = 0
  wm[:, :, c8:, :] = 0
  return E.expect_plain(_conv(op, x=x, wm=wm)['y']), E.expect_plain(ref['y'])


def _m_cout_tail(op, ref):
  """A direct dgrad whose reduction over the output columns runs in whole groups of 8: the last cout % 8 columns are left out."""
  c8 = op.case[4] - op.case[4] % 8
  if c8 == op.case[4]:
    return None
  wm, dy = op.wm.clone(), op.dy.clone()
  wm[..., c8:] = 0
  dy[..., c8:] = 0
  return E.expect_plain(_conv(op, wm=wm, dy=dy, want=('y', 'dx'))['dx']), E.expect_plain(ref['dx'])


def _m_same_tap(op, ref):
  """A stride-2 3x3 without leading padding (TF SAME on an even size: pad 0 in front, 1 behind) taken for a window that ends
  where the image ends: the bottom row and the right column of the filter are never applied."""
  N, H, W, Cin, Cout, k, stride, pt, pl, Ho, Wo = op.case
  if not (k == 3 and stride == 2 and pt == 0 and pl == 0):
    return None
  wm = op.wm.clone()
  wm[2, :] = 0
  wm[:, 2] = 0
  return E.expect_plain(_conv(op, wm=wm)['y']), E.expect_plain(ref['y'])


def _m_parity_unwritten(op, ref):
  """A strided 1x1 dgrad that writes the pixels the conv read and leaves the other parity classes as it found them (the
  sentinel of the guarded output) instead of writing their zeros."""
  N, H, W, Cin, Cout, k, stride, pt, pl, Ho, Wo = op.case
  if not (k == 1 and stride > 1):
    return None
  want = E.expect_plain(ref['dx'])
  got = torch.full_like(want, E.SENTINEL16)
  got[:, ::stride, ::stride, :] = want[:, ::stride, ::stride, :]
  assert float(ref['dx'][:, 1::stride].abs().max()) == 0.0
  return got, want


def _m_one_rounding(op, ref):
  """The host fallback adding the addend before the first rounding: bf16(dgrad + addend), one rounding instead of two."""
  add = op.add.double()
  return E.rne_bits(ref['dx'] + add), E.expect_acc(ref['dx'], add)


MUTANTS = {'cin_tail': _m_cin_tail, 'cout_tail': _m_cout_tail, 'same_tap': _m_same_tap, 'parity_unwritten': _m_parity_unwritten,
           'one_rounding': _m_one_rounding}
SHAPE_MUTANTS = ('cin_tail', 'cout_tail', 'same_tap', 'parity_unwritten')    # those that act on a property of the shape


@functools.lru_cache(maxsize=None)
def _rejections(name, regime):
  """{mutant: indices of the cases of the set whose bit comparison rejects it}."""
  out = {m: [] for m in MUTANTS}
  for i in range(len(SETS[name])):
    op, ref, _ = _case(name, i, regime)
    for m, fn in MUTANTS.items():
      pair = fn(op, ref)
      if pair is None:
        continue
      try:
        E.assert_bits(m, pair[0], pair[1])
      except AssertionError as err:
        assert 'differ in bits' in str(err)
        out[m].append(i)
  return out


@pytest.mark.parametrize('regime', REGIMES)
def test_every_mutant_is_rejected_in_both_regimes(regime):
  rej = {name: _rejections(name, regime) for name in SETS}
  for m in SHAPE_MUTANTS:
    assert any(rej[name][m] for name in SETS), (m, regime)
  # every case a shape mutant applies to rejects it: a dropped term changes the bits whatever its size
  for name, cases in SETS.items():
    for m in SHAPE_MUTANTS:
      applies = [i for i, c in enumerate(cases) if MUTANTS[m](*_case(name, i, regime)[:2]) is not None]
      assert rej[name][m] == applies, (name, m, regime, rej[name][m], applies)
  if regime == 'round':
    # one rounding instead of two shows wherever the first rounding rounds: every case of every set
    for name, cases in SETS.items():
      assert rej[name]['one_rounding'] == list(range(len(cases))), (name, rej[name]['one_rounding'])
  else:
    # 'low': |dx| <= 256 units is exactly bf16, so the first rounding changes nothing and the two forms are the SAME function
    # of these operands -- by construction no operand of this regime can tell them apart; 'round' is where it is told
    for name in SETS:
      assert rej[name]['one_rounding'] == []


@pytest.mark.parametrize('regime', REGIMES)
def test_each_set_rejects_a_mutant_the_small_set_cannot(regime):
  """No shape mutant applies to any case of k1_check.SMALL_CASES (channel counts in multiples of 8, stride 1, no strided 1x1):
  there the mutant IS the kernel, so `small` cannot reject it, whatever the operands."""
  for i, c in enumerate(k1_check.SMALL_CASES):
    N, H, W, Cin, Cout, k, stride, pt, pl, Ho, Wo = c
    assert Cin % 8 == 0 and Cout % 8 == 0 and stride == 1
  probe = E.operands(k1_check.SMALL_CASES[0], 100, regime)
  pref, _ = E.reference(probe)
  assert all(MUTANTS[m](probe, pref) is None for m in SHAPE_MUTANTS)
  want = {'wrn': {'cin_tail', 'same_tap', 'parity_unwritten'}, 'mlp': {'cin_tail', 'cout_tail'},
          'odd': {'cin_tail', 'cout_tail', 'same_tap', 'parity_unwritten'}}
  for name in SETS:
    got = {m for m in SHAPE_MUTANTS if _rejections(name, regime)[m]}
    assert got and got == want[name], (name, regime, got)


# ---- drift ----------------------------------------------------------------------------------------------------------------
def _wrn_shapes(width):
  """Every masked conv / dense layer of WideResNet-22 on a 32 x 32 input as a case without its batch, from the workload built
  on the CPU: the descriptors its own layers make."""
  from rigl_amd import variables as V
  from rigl_amd.workloads import wide_resnet
  m = wide_resnet.WideResNet(V.Graph('cpu'), depth=22, width=width)

  def shape(layer, hw):
    d = layer.desc_for(1, hw, hw)
    assert d.kh == d.kw and d.stride_h == d.stride_w and d.h == d.w == hw and d.ho == d.wo
    return (d.h, d.w, d.cin, d.cout, d.kh, d.stride_h, d.pad_top, d.pad_left, d.ho, d.wo)

  out, hw = [shape(m.stem, 32)], 32
  for b in m.blocks:
    if 'skip' in b:
      out.append(shape(b['skip'], hw))
    out.append(shape(b['conv1'], hw))
    hw = out[-1][-1]
    out.append(shape(b['conv2'], hw))
  assert hw == 8
  out.append((1, 1, m.logits.n_in, m.logits.units, 1, 1, 0, 0, 1, 1))
  return sorted(set(out))


def _held():
  return {c[1:] for cases in SETS.values() for c in cases}


def test_the_sets_hold_every_layer_of_the_mnist_mlp():
  from rigl_amd import variables as V
  from rigl_amd.workloads import mnist_mlp
  m = mnist_mlp.MnistMLP(V.Graph('cpu'))
  shapes = [(1, 1, l.n_in, l.units, 1, 1, 0, 0, 1, 1) for l in m.layers]
  assert [s[2:4] for s in shapes] == [(784, 300), (300, 100), (100, 10)]
  assert set(shapes) <= _held()
  assert set(shapes) <= {c[1:] for c in k1_check.MLP_CASES}


def test_the_sets_hold_every_layer_of_wide_resnet_22():
  """Width 1 (BASELINE config 2): every layer, at its own spatial size.  A changed workload fails here."""
  shapes = _wrn_shapes(1)
  assert len(shapes) == 9               # the stem, three stages of (first 3x3, 3x3), two strided skips, the logits
  missing = [s for s in shapes if s not in _held()]
  assert not missing, missing


# Width 2: the ten wrn cases carry its 128 -> 128 layer, its stride-1 1x1 skip and its logits; its other layers have the channel
# pairs of width 1 one stage earlier, i.e. at twice the spatial size, and two pairs (16 -> 32 and 64 -> 128) at a stride the
# sets hold only for other channel counts.  They are listed here so that the split is pinned: held + listed == the workload.
WRN22_WIDTH2_NOT_HELD = [
    (32, 32, 16, 32, 3, 1, 1, 1, 32, 32), (32, 32, 32, 32, 3, 1, 1, 1, 32, 32),
    (32, 32, 32, 64, 1, 2, 0, 0, 16, 16), (32, 32, 32, 64, 3, 2, 0, 0, 16, 16), (16, 16, 64, 64, 3, 1, 1, 1, 16, 16),
    (16, 16, 64, 128, 1, 2, 0, 0, 8, 8), (16, 16, 64, 128, 3, 2, 0, 0, 8, 8),
]


def test_wide_resnet_22_width_2_against_the_sets():
  shapes = _wrn_shapes(2)
  held = [s for s in shapes if s in _held()]
  assert sorted(held + WRN22_WIDTH2_NOT_HELD) == shapes
  assert {(s[2], s[3]) for s in held} == {(3, 16), (16, 32), (128, 128), (128, 10)}
  # what is not held at its own size is held in kind: the same kernel size, stride and padding, at channel counts whose
  # residues modulo 8 and K-block counts (16, 32, 64, 128) the sets walk
  kinds = {(c[5], c[6], c[7], c[8]) for c in k1_check.WRN_CASES}
  assert {(s[4], s[5], s[6], s[7]) for s in WRN22_WIDTH2_NOT_HELD} <= kinds


# ---- descriptor validation of the direct entry points (host code: refused before anything touches the device) ---------------
def test_the_direct_entry_points_validate_their_descriptors():
  """The bad descriptors of tests/test_conv_ref_refusals_gpu.py on host pointers: check_desc answers before a pointer is used
  or the device is asked for anything, so the codes can be pinned without a GPU (the GPU test adds the untouched outputs and
  the valid neighbours)."""
  import ctypes as C
  from rigl_amd import _lib
  from tests import test_conv_ref_refusals_gpu as R
  lib = _lib.load()
  buf = torch.zeros(256)
  for what, over, code in R.BAD + [(w, f, 'EUNSUPPORTED') for w, f in R.HUGE]:
    d = R._desc(R.BASE, **over)
    for fn in (lib.rigl_conv2d_fwd_ref, lib.rigl_conv2d_dgrad_ref, lib.rigl_conv2d_wgrad_ref):
      rc = fn(C.byref(d), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), None)
      assert rc == getattr(_lib, 'RIGL_' + code), (what, rc, lib.rigl_last_error())
  assert bool((buf == 0).all())
