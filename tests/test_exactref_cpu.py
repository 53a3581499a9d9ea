"""tests/exactref.py checked without a GPU: the integer bf16 rounding against hand-written ties, the operand generators
against the input conditions of both regimes (on the small case lists by running the fp64 reference, at the batch-128
shapes from the plan alone), and MUTANTS -- the exact expected tensor damaged the way a subtly wrong kernel would damage it
(truncation, round-half-away, a double rounding, a dropped tap, a dropped row of one statistics part, a store one element
past the end) -- each of which the bit comparison or the guard check must reject, while the tolerance of
tests/convref.check_close accepts round-half-away."""
import numpy as np
import pytest
import torch

from tests import convref
from tests import exactref as E
from tests import k1_check


# ---- the rounding -------------------------------------------------------------------------------------------------------
# value, bf16 pattern under round-to-nearest-even (worked by hand: bf16 keeps 8 significant bits)
HAND = [
    (1.0, 0x3F80),
    (1.0 + 2.0 ** -8, 0x3F80),            # tie between 1 and 1 + 2^-7: down to the even 0x3F80
    (1.0 + 3 * 2.0 ** -8, 0x3F82),        # tie between 0x3F81 and 0x3F82: up to the even one
    (-(1.0 + 2.0 ** -8), 0xBF80),         # the same two with the sign set: magnitudes round alike
    (-(1.0 + 3 * 2.0 ** -8), 0xBF82),
    (257.0, 0x4380),                      # 256 | 258: tie, 256 = 0x4380 is even
    (259.0, 0x4382),                      # 258 | 260: tie, 260 = 0x4382 is even
    (-257.0, 0xC380),
    (-259.0, 0xC382),
    (258.0, 0x4381),                      # exactly representable, odd pattern
    (511.0, 0x4400),                      # 510 | 512: tie, up across the binade to 512
    (1026.0, 0x4480),                     # 1024 | 1032: below the tie at 1028
    (1028.0, 0x4480),                     # the tie: down to even 1024
    (1030.0, 0x4481),                     # above it
    (1036.0, 0x4482),                     # 1032 | 1040: tie, 1040 = 0x4482 is even
    (257 * 2.0 ** -5, 0x4100),            # a unit of 2^-5: the tie 257 again, three binades down (8.03125 -> 8)
    (0.0, 0x0000),
    (-0.0, 0x0000),                       # an exact zero is +0
]


def test_rne_against_hand_written_ties():
  v = np.array([h[0] for h in HAND], dtype=np.float64)
  want = np.array([h[1] for h in HAND], dtype=np.int64)
  np.testing.assert_array_equal(E.rne_bits(v), want)
  np.testing.assert_array_equal(E.rne_bits(torch.from_numpy(v)).numpy(), want)
  # the other modes on the two directions of a tie
  assert E.rne_bits(np.array([257.0, 259.0, -257.0]), 'rha').tolist() == [0x4381, 0x4382, 0xC381]
  assert E.rne_bits(np.array([257.0, 259.0, -259.0]), 'trunc').tolist() == [0x4380, 0x4381, 0xC381]
  np.testing.assert_array_equal(E.bits_value(want[:15]), [1, 1, 1 + 2.0 ** -6, -1, -(1 + 2.0 ** -6), 256, 260, -256, -260, 258,
                                                          512, 1024, 1024, 1032, 1040])


def test_two_step_addend_form():
  """bf16(bf16(dgrad) + addend) is NOT bf16(dgrad + addend): 257 rounds to 256 first, + 1 = 257 rounds to 256 again, while
  258 is representable; and 259 -> 260, + 1 = 261 -> 260 | 262 tie -> even 0x4382 = 260, while 260 + ... one rounding of 260
  would agree -- the addend meets the ROUNDED gradient."""
  got = E.expect_acc(np.array([257.0, 259.0, -257.0, 255.0]), np.array([1.0, 1.0, -1.0, 0.5]))
  assert got.tolist() == [0x4380, 0x4382, 0xC380, 0x4380]               # 255 + 0.5: 255 | 256 tie -> even 256
  assert E.rne_bits(np.array([258.0])).tolist() == [0x4381]
  t = E.expect_acc(torch.tensor([257.0, 259.0, -257.0, 255.0], dtype=torch.float64), torch.tensor([1.0, 1.0, -1.0, 0.5],
                                                                                                  dtype=torch.float64))
  assert t.tolist() == got.tolist()


def test_numpy_and_torch_paths_and_every_integer():
  """All integers up to 2^17 in both signs and three units: the NumPy and the torch expressions agree, the result is within
  half a bf16 step of the value, and a value exactly between two bf16 neighbours went to the even one."""
  v = np.arange(-(1 << 17), (1 << 17) + 1, dtype=np.float64)
  for unit in (1.0, 0.25, 2.0 ** -5):
    a = v * unit
    b = E.rne_bits(a)
    np.testing.assert_array_equal(E.rne_bits(torch.from_numpy(a)).numpy(), b)
    r = E.bits_value(b)
    np.testing.assert_array_equal(E.bits_value(torch.from_numpy(b)).numpy(), r)
    step = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(a), 2.0 ** -100))) - 7)
    assert (np.abs(r - a) <= step / 2).all()
    tie = np.abs(r - a) == step / 2
    assert tie.any() and (b[tie] & 1 == 0).all()
    t, up, dn = E.tie_shares(a, unit)
    assert abs(t - tie.mean()) < 1e-12 and up > 0 and dn > 0


# ---- the generators -----------------------------------------------------------------------------------------------------
SMALL_LISTS = [('small', k1_check.SMALL_CASES), ('pp', k1_check.PP_CASES), ('c3', k1_check.C3_CASES), ('stem', k1_check.STEM_CASES)]


@pytest.mark.parametrize('name,cases', SMALL_LISTS, ids=[n for n, _ in SMALL_LISTS])
@pytest.mark.parametrize('regime', ['low', 'round'])
def test_input_conditions_on_the_small_case_lists(name, cases, regime):
  """The runner's seeds (100 + i), the fp64 reference on the CPU: integer multiples of the unit, sum|a||b| <= 2^24, and the
  regime's own conditions (check_conditions asserts them); every value exact in bf16; the unit is not always 1."""
  js = set()
  for i, c in enumerate(cases):
    op = E.operands(c, 100 + i, regime)
    for t in (op.x, op.dy, op.wm, op.add):
      assert torch.equal(t.to(torch.bfloat16).float(), t)
    assert float((op.x / op.ux).abs().max()) <= 256 and float((op.wm / op.uw).abs().max()) <= 256
    assert (op.m01 is not None) == (i % 2 == 1)
    if op.m01 is not None:
      assert 0.15 < float(op.m01.mean()) < 0.25
    js.add((op.ux, op.uw, op.ud))
    ref, ab = E.reference(op, ('y', 'dx', 'dw') if c[3] % 8 == 0 else ('y', 'dw'))
    fig = E.check_conditions(op, ref, ab)
    if regime == 'round':
      assert 300 <= fig['std_y'] <= 1000
  assert len(js) > 1 and any(u != (1.0, 1.0, 1.0) for u in js)


def _big_shapes():
  """(case, depthwise, masked) of the runner's large sets: the mask goes with the odd seeds 100 + i, as in the runner."""
  from tests import test_k3_k1_gpu as T
  from tests.test_vgg_gpu import C3_SHAPES, VGG16_SHAPES
  out = []
  for cases in (k1_check.resnet50_shapes(128), k1_check.mobilenet_v1_shapes(128), k1_check.RS_CASES, k1_check.BS_CASES,
                [(n, h, w, ci, co, 3, 1, 1, 1, h, w) for n, h, w, ci, co in VGG16_SHAPES + C3_SHAPES]):
    out += [(c, False, i % 2 == 1) for i, c in enumerate(cases)]
  out += [((128, hw, hw, c, c, 3, s, 1, 1, (hw - 1) // s + 1, (hw - 1) // s + 1), True, False) for hw, c, s in T.MOBILENET_V1_DEPTHWISE]
  return out


@pytest.mark.parametrize('regime', ['low', 'round'])
def test_plans_at_the_batch_128_shapes(regime):
  """Without running the reference: the worst case of the plan (every element at its amplitude, every position taken) keeps
  sum|a||b| within 2^24 units for y, dx and dw, and what the plan aims at lies inside the regime -- 'round': both stds in
  300 .. 1000 units; 'low': E[y^2] <= 400 (|y| <= 256 is 12 sigma away) and rows * E[y^2] <= 2^24 / 4.  The GPU runner asserts
  the conditions themselves on the reference of every case it runs."""
  for case, depthwise, masked in _big_shapes():
    p = E.plan(case, regime, masked, depthwise)
    wc = E.worst_case(case, p, depthwise)
    assert max(wc.values()) <= E.LIMIT, (case, p, wc)
    assert p['ax'] <= 3 and p['ad'] <= 3 and p['aw'] <= 255
    m = E.expected_moments(case, p, depthwise)
    has_dx = depthwise or case[3] % 8 == 0
    if regime == 'round':
      assert 300 <= m['y2'] ** 0.5 <= 1000, (case, p, m)
      assert not has_dx or 300 <= m['dx2'] ** 0.5 <= 1000, (case, p, m)
    else:
      rows = case[0] * case[9] * case[10]
      assert m['y2'] <= 400.0 * 1.0001 and rows * m['y2'] <= E.LIMIT / 4 * 1.0001, (case, p, m)
      assert not has_dx or m['dx2'] <= 400.0 * 1.0001, (case, p, m)


# ---- mutants --------------------------------------------------------------------------------------------------------------
CASE = (2, 14, 14, 64, 256, 3, 1, 1, 1, 14, 14)        # the issue's measured case (3x3, 64 -> 256)


def _exact(regime, seed=101):
  op = E.operands(CASE, seed, regime)
  ref, ab = E.reference(op)
  E.check_conditions(op, ref, ab)
  return op, ref, ab


def _rejected(name, got, want):
  with pytest.raises(AssertionError, match='differ in bits'):
    E.assert_bits(name, got, want)


def test_rounding_mutants_are_rejected_and_the_tolerance_accepts_half_away():
  op, ref, ab = _exact('round')
  for key in ('y', 'dx'):
    exact = ref[key].numpy()
    want = E.expect_plain(exact)
    E.assert_bits(key, E.rne_bits(torch.from_numpy(exact)).numpy(), want)          # (the comparison itself passes on equal bits)
    rha, trunc = E.rne_bits(exact, 'rha'), E.rne_bits(exact, 'trunc')
    _rejected(key + ' half-away', rha, want)
    _rejected(key + ' truncation', trunc, want)
    # round-half-away differs exactly on the ties that round down to even: >= 2 % of the elements
    assert (rha != want).mean() >= 0.02
    # ... and the Gaussian-operand bound of the existing suite cannot see it (nor could it on these operands)
    convref.check_close(key, torch.from_numpy(E.bits_value(rha)), ref[key], ab[key], 1e-5, 2.0 ** -8)
  # a double rounding through an fp16-wide (11 significant bits) intermediate: needs values of 12+ bits -- the wider dX here
  # has few, so an integer ramp up to 2^17 stands in for a longer reduction
  ramp = np.arange(-(1 << 17), (1 << 17) + 1, dtype=np.float64) * op.udx
  _rejected('double rounding', E.double_rounded_bits(ramp), E.expect_plain(ramp))
  assert E.double_rounded_bits(np.array([4113.0])).tolist() != E.rne_bits(np.array([4113.0])).tolist()
  # the two-step addend form rounded once instead of twice
  add = op.add.double().numpy()
  _rejected('one rounding of dgrad + addend', E.rne_bits(ref['dx'].numpy() + add), E.expect_acc(ref['dx'].numpy(), add))


@pytest.mark.parametrize('regime', ['low', 'round'])
def test_a_dropped_tap_is_rejected(regime):
  """One filter tap of one (input, output) channel pair left out -- a single term of the 576: the output elements of that
  channel it reaches have other bits, whatever the term's size."""
  op, ref, ab = _exact(regime)
  nz = (op.wm[1, 1] != 0).nonzero()[0]
  ci, co = int(nz[0]), int(nz[1])
  op.wm = op.wm.clone()
  op.wm[1, 1, ci, co] = 0
  bad, _ = E.reference(op, ('y',))
  _rejected('dropped tap', E.expect_plain(bad['y'].numpy()), E.expect_plain(ref['y'].numpy()))


def test_a_dropped_row_in_one_statistics_part_is_rejected():
  """'low': any partition of the rows sums exactly in fp32, so the partials must add up to the exact totals -- leave one row
  out of one part and the equality fails, for sum y and for sum y^2 (the relative bound of the tolerance suite, 2e-6, lets
  a row of 392 pass whenever the column total is large)."""
  op, ref, _ = _exact('low')
  y = ref['y'].reshape(-1, CASE[4])
  tot = (y.sum(0), (y * y).sum(0))
  rows = 128
  parts = [y[r:r + rows] for r in range(0, y.shape[0], rows)]
  def partials(ps):
    return torch.stack([torch.stack([p.float().sum(0), (p.float() * p.float()).sum(0)]) for p in ps])
  s = partials(parts).double().sum(0)
  assert torch.equal(s[0], tot[0]) and torch.equal(s[1], tot[1])
  row = int((parts[1].abs().sum(1) > 0).nonzero()[0])
  parts[1] = torch.cat([parts[1][:row], parts[1][row + 1:]])
  s = partials(parts).double().sum(0)
  assert not torch.equal(s[0], tot[0]) or not torch.equal(s[1], tot[1])
  assert not torch.equal(s[1], tot[1])


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_guard_bands(dtype):
  shape = (3, 5, 7, 24)
  out, check, buf = E.guarded(shape, dtype, 'cpu')
  n = out.numel()
  g = (buf.numel() - n) // 2
  assert g >= E.GUARD_ROWS * shape[-1] and out.data_ptr() % 256 == buf.data_ptr() % 256
  assert out.shape == shape and out.dtype == dtype and out.is_contiguous()
  sent = E.SENTINEL16 if dtype == torch.bfloat16 else E.SENTINEL32
  assert int(buf[0]) == sent and int(buf[-1]) == sent and int(buf[g]) == sent
  with pytest.raises(AssertionError, match='never written'):
    check('untouched')
  out.fill_(1.0)
  check('whole')
  buf[g + n - 1] = sent                                              # a skipped last element
  with pytest.raises(AssertionError, match=r'1 / %d output elements never written, first at flat index %d' % (n, n - 1)):
    check('last element skipped')
  out.fill_(1.0)
  buf[g + n] = 0                                                     # a store one element past the end
  with pytest.raises(AssertionError, match=r'behind the output: 1 guard elements touched, first at offset %d ' % n):
    check('one past the end')
  buf[g + n] = sent
  buf[g - 1] = 0                                                     # ... and one in front
  with pytest.raises(AssertionError, match=r'in front of the output: 1 guard elements touched, first at offset -1 '):
    check('one in front')
  buf[g - 1] = sent
  buf[g + n + 24 * 6 + 3] = 0                                        # a ragged tile's seventh extra row
  with pytest.raises(AssertionError, match=r'first at offset %d ' % (n + 24 * 6 + 3)):
    check('a row past the end')
