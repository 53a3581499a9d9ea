"""NumPy reference of rigl_grad_accumulate_ranges (include/rigl_hip.h) and the seeded cases its tests run, built on
tests/accum_ref.py: the same buffer of 32-bit words -- both arenas of ``n`` elements between poisoned guards, the three loss
scalars between poisoned words -- with every arena element OUTSIDE the case's ranges poisoned too, in both arenas: a gap between
two ranges, the elements in front of the first and behind the last range are guards like the ones around the arenas.  The
poison of an arena's gaps, of its slack and of the 32 words on either side of it is a FINITE pattern of its own (POISON_ACC,
POISON_G): a copy or a sum of the two arenas' poisons is neither of them, so a pass that strays outside its ranges changes bits
(all-ones words are NaN in both arenas, and NaN + NaN leaves the all-ones word it found).

An implementation is a callable ``impl(buf, lay, ranges, mode, inv_k, max_blocks)`` that works on the uint32 array in place;
``ranges`` is a list of ``(offset, length)`` in elements.  ``reference`` is the one the kernel is held to: per element of every
range the arithmetic of accum_ref.reference, the loss arithmetic once per call whatever the table holds.  ``check_stage`` runs ONE
mode from the state the reference leaves in front of it, ``check_chain`` FIRST, ADD, LAST over the case's three gradients; both
return the list of complaints (empty: the implementation passed).
"""
import numpy as np

import accum_ref as A

F32, U32 = A.F32, A.U32
FIRST, ADD, LAST = A.FIRST, A.ADD, A.LAST
MODES = A.MODES
POISON = A.POISON
POISON_ACC = U32(0xDEADBEEF)       # -6.26e18
POISON_G = U32(0x4B3C614E)         # 12345678.0
NEAR = 32                          # words of an arena's own poison on either side of it
TILE = A.TILE
MAX_BLOCKS = A.MAX_BLOCKS          # 0: the default grid
MAX_RANGES = 8                     # rigl_amd._lib.ACC_MAX_RANGES
LENGTHS = (0, 1, 3, 4, 5, TILE - 1, TILE, TILE + 1)
INV_K = 1.0 / 3


def reference(buf, lay, ranges, mode, inv_k, max_blocks=0):
  del max_blocks                                     # the result depends on the operands alone
  a, g = lay['acc'], lay['g']
  for off, ln in ranges:
    sa, sg = slice(a + off, a + off + ln), slice(g + off, g + off + ln)
    if mode == FIRST:
      buf[sa] = buf[sg]
    elif mode == ADD:
      buf[sa] = A.add32(buf[sa], buf[sg])
    else:
      buf[sg] = A.add32(buf[sa], buf[sg])
  loss_arithmetic(buf, lay, mode, inv_k)


def loss_arithmetic(buf, lay, mode, inv_k):
  l, la, lm = lay['loss'], lay['loss_acc'], lay['loss_mean']
  if mode == FIRST:
    buf[la] = buf[l]
  elif mode == ADD:
    buf[la] = A.add32(buf[la:la + 1], buf[l:l + 1])[0]
  else:
    s = A.floats(A.add32(buf[la:la + 1], buf[l:l + 1]))
    with np.errstate(all='ignore'):
      buf[lm] = A.bits(s * F32(inv_k))[0]


def fused_mean(l1, l2, l3, inv_k=INV_K):
  """The mean an FMA would leave: fl(loss_acc * inv_k + fl(l3 * inv_k)), the first product unrounded (exact in fp64)."""
  la = F32(F32(l1) + F32(l2))
  p = F32(F32(l3) * F32(inv_k))
  return int(A.bits(F32(np.float64(la) * np.float64(F32(inv_k)) + np.float64(p)))[0])


def _loss_triples(rng, count):
  """Three losses whose mean tells the kernel's two roundings from a division, from one rounding of the fp64 mean and from
  the fused form above."""
  out = []
  while len(out) < count:
    l = tuple((rng.random(3) * 3.0 + 0.5).astype(F32))
    m, d, w = A.loss_variants(*l)
    if m != d and m != w and m != fused_mean(*l):
      out.append(l)
  return out


# ---- cases -------------------------------------------------------------------------------------------------------------------
def place(lengths, gaps, lead=0):
  """Ranges of the given lengths: the first at ``lead``, each next one ``gap`` elements behind the end of the one in front
  rounded up to a multiple of 4 (gap 0 and a length that is a multiple of 4: the two touch)."""
  out, off = [], lead
  for i, ln in enumerate(lengths):
    out.append((off, ln))
    off = -(-(off + ln) // 4) * 4 + (gaps[i] if i < len(gaps) else 0)
  return out


def inside_mask(n, ranges):
  m = np.zeros(n, dtype=bool)
  for off, ln in ranges:
    m[off:off + ln] = True
  return m


def build_cases(seed=20260202):
  """The list of cases: dicts with 'name', 'n', 'ranges', 'stale' (what acc holds before FIRST: [n] bit patterns, used
  inside the ranges only), 'g' ([3][n], likewise), 'special' (the bit-pattern columns written at the start of the ranges' elements,
  or None) and 'loss' (three fp32)."""
  rng = np.random.default_rng(seed)
  cols = A._special_columns(rng)                     # pylint: disable=protected-access
  every = np.concatenate(list(cols.values()))
  losses = _loss_triples(rng, 4)
  cases = []

  def case(name, ranges, n=None, special=None):
    end = max([o + l for o, l in ranges] + [0])
    n = end if n is None else n                      # default: the last range ends at n
    assert n >= end
    m = inside_mask(n, ranges)
    k = int(m.sum())
    g = np.full((3, n), POISON, dtype=U32)
    stale = np.full(n, POISON, dtype=U32)
    for i in range(3):
      g[i, m] = A._random_bits(rng, k)               # pylint: disable=protected-access
    stale[m] = A._random_bits(rng, k)                # pylint: disable=protected-access
    if special is not None:
      idx = np.flatnonzero(m)[:len(special)]
      g[:, idx] = special[:len(idx)].T
    cases.append(dict(name=name, n=n, ranges=list(ranges), stale=stale, g=g, special=special,
                      loss=losses[len(cases) % len(losses)]))

  for ln in LENGTHS:                                 # one range of every length: in the middle of an arena, and ending at n
    case('one_%d_inside' % ln, [(8, ln)], n=8 + ln + 9)
    case('one_%d_to_n' % ln, [(8, ln)])
  case('two_touching', place([TILE, 5], [0]), n=TILE + 64)
  case('two_touching_to_n', place([8, TILE + 4], [0], lead=4))
  case('two_gap4', place([TILE - 1, TILE + 1], [4]), n=2 * TILE + 70)
  case('two_empty', place([0, 0], [4], lead=12), n=64)
  case('eight_every_length', place(LENGTHS, [0, 4, 0, 4, 0, 4, 0]))
  case('eight_every_length_reversed', place(LENGTHS[::-1], [4, 0, 4, 0, 4, 0, 4], lead=64), n=64 + 3 * TILE + 200)
  case('eight_touching', place([4, TILE, 8, 0, 4, 2 * TILE, 4, 12], [0] * 7))
  case('eight_gap4', place([4, 5, 1, 3, 4, 4, 7, 8], [4] * 7, lead=4), n=128)
  # the final flush of a data-parallel step: a long head, a short tail that ends at n; whole tiles that start off a tile boundary
  case('head_and_tail', [(0, 5 * TILE + 100), (7 * TILE + 64, 203)])
  case('short_then_long', place([20, 3 * TILE + 6], [0]), n=3 * TILE + 64)
  case('whole_arena', [(0, 2 * TILE + A.WAVE + 7)])
  case('specials_two_odd', place([len(every) // 2 | 1, len(every)], [4], lead=4), special=every)
  for name, col in cols.items():
    reps = np.concatenate([col] * -(-7 // len(col)))
    case('specials_' + name, place([3, len(reps) - 3 | 1], [4]), special=reps)
  case('empty_table_with_loss', [], n=64)
  return cases


def poisoned(lay):
  """The buffer with nothing live in it."""
  buf = np.full(lay['total'], POISON, dtype=U32)
  buf[lay['acc'] - NEAR:lay['acc'] + lay['pad'] + NEAR] = POISON_ACC
  buf[lay['g'] - NEAR:lay['g'] + lay['pad'] + NEAR] = POISON_G
  return buf


def load_gradient(buf, lay, case, i):
  m = inside_mask(case['n'], case['ranges'])
  buf[lay['g']:lay['g'] + case['n']][m] = case['g'][i][m]
  buf[lay['loss']] = int(A.bits(case['loss'][i])[0])


def state_before(case, mode):
  """The buffer in front of stage ``mode`` of the case's chain, as the reference leaves it, and its layout."""
  lay = A.layout(case['n'])
  assert NEAR <= A.GUARD // 2
  buf = poisoned(lay)
  m = inside_mask(case['n'], case['ranges'])
  buf[lay['acc']:lay['acc'] + case['n']][m] = case['stale'][m]
  buf[lay['loss_acc']], buf[lay['loss_mean']] = 0x40A00000, 0x40C00000                 # stale: 5.0, 6.0
  load_gradient(buf, lay, case, 0)
  for i in range(mode):
    reference(buf, lay, case['ranges'], i, INV_K)
    load_gradient(buf, lay, case, i + 1)
  return buf, lay


def written_mask(lay, ranges, mode):
  """The words stage ``mode`` writes: the ranges of its destination arena and its loss scalar."""
  w = np.zeros(lay['total'], dtype=bool)
  dst = lay['g'] if mode == LAST else lay['acc']
  w[dst:dst + lay['n']] = inside_mask(lay['n'], ranges)
  w[lay['loss_mean'] if mode == LAST else lay['loss_acc']] = True
  return w


def compare(got, want, lay, ranges, modes):
  """Complaints of ``got`` against ``want``: zero differing bits everywhere; only inside what a stage that ADDS writes may a
  NaN differ in its payload, and must still be a NaN."""
  out = []
  differ = got != want
  inside = np.zeros(len(want), dtype=bool)
  nan_ok = np.zeros(len(want), dtype=bool)
  for mode in modes:
    w = written_mask(lay, ranges, mode)
    inside |= w
    if mode != FIRST:
      nan_ok |= w
  differ &= ~(nan_ok & A.is_nan(want) & A.is_nan(got))
  if np.any(differ & inside):
    i = int(np.flatnonzero(differ & inside)[0])
    out.append('value: word %d is %08x, expected %08x (%d words differ)' % (i, got[i], want[i], int(np.sum(differ & inside))))
  if np.any(differ & ~inside):
    i = int(np.flatnonzero(differ & ~inside)[0])
    out.append('untouched: word %d (guard / gap / slack / unwritten operand) is %08x, was %08x' % (i, got[i], want[i]))
  return out


def check_stage(impl, case, mode, max_blocks=0):
  before, lay = state_before(case, mode)
  want = before.copy()
  reference(want, lay, case['ranges'], mode, INV_K)
  got = before.copy()
  impl(got, lay, case['ranges'], mode, INV_K, max_blocks)
  out = compare(got, want, lay, case['ranges'], [mode])
  again = before.copy()
  impl(again, lay, case['ranges'], mode, INV_K, max_blocks)
  if not np.array_equal(again, got):
    out.append('repeat: a second run from the same state differs')
  return out


def check_chain(impl, case, max_blocks=0):
  """FIRST, ADD, LAST over the case's three gradients and losses; the end state against the reference's."""
  results = []
  for f in (impl, reference):
    buf, lay = state_before(case, FIRST)
    for m in MODES:
      if m:
        load_gradient(buf, lay, case, m)
      f(buf, lay, case['ranges'], m, INV_K, max_blocks)
    results.append(buf)
  return compare(results[0], results[1], lay, case['ranges'], [ADD, LAST])
