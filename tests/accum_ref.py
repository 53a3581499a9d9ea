"""NumPy reference of rigl_grad_accumulate (include/rigl_hip.h) and the seeded cases its tests run.

One buffer of 32-bit words holds both operands between poisoned guards (every byte 0xFF), the slack between ``n`` and the next
64-element boundary poisoned too, and the three loss scalars between poisoned words:

  [guard 64][acc: n | slack][guard 64][grad: n | slack][guard 64][P loss P loss_acc P loss_mean P P]

An implementation is a callable ``impl(buf, lay, mode, inv_k, max_blocks)`` that works on the uint32 array in place; ``reference``
is the one the kernel is held to: one fp32 addition per element, FIRST a copy, the loss sum and the product with inv_k rounded
separately.  ``check_stage`` runs ONE mode from the state the reference leaves in front of it, ``check_chain`` runs FIRST, ADD,
LAST over a case's three gradients; both return the list of complaints (empty: the implementation passed).
"""
import numpy as np

F32 = np.float32
U32 = np.uint32
FIRST, ADD, LAST = 0, 1, 2
MODES = (FIRST, ADD, LAST)
GUARD = 64
POISON = U32(0xFFFFFFFF)
WAVE = 64 * 4                 # elements one wave's 16-byte vector access covers
TILE = 256 * 4 * 4            # elements per block and iteration (rigl_amd._lib.ACC_TILE)
MAX_BLOCKS = (0, 1, 3)        # 0: the default grid
FLT_MAX = 0x7F7FFFFF


def bits(x):
  return np.ascontiguousarray(np.asarray(x, dtype=F32)).view(U32).copy()


def floats(b):
  return np.ascontiguousarray(np.asarray(b, dtype=U32)).view(F32)


def add32(a, b):
  """fl(a + b), element-wise on bit patterns: one IEEE fp32 addition, subnormals kept."""
  with np.errstate(all='ignore'):
    return bits(floats(a) + floats(b))


def is_nan(b):
  b = np.asarray(b, dtype=U32)
  return (b & U32(0x7FFFFFFF)) > U32(0x7F800000)


def layout(n):
  pad = -(-n // 64) * 64
  acc = GUARD
  g = acc + pad + GUARD
  scal = g + pad + GUARD
  return dict(n=n, pad=pad, acc=acc, g=g, loss=scal + 1, loss_acc=scal + 3, loss_mean=scal + 5, total=scal + 8)


def make_buffer(lay, acc_bits, g_bits, loss, loss_acc, loss_mean):
  buf = np.full(lay['total'], POISON, dtype=U32)
  n = lay['n']
  buf[lay['acc']:lay['acc'] + n] = acc_bits
  buf[lay['g']:lay['g'] + n] = g_bits
  buf[lay['loss']], buf[lay['loss_acc']], buf[lay['loss_mean']] = loss, loss_acc, loss_mean
  return buf


def reference(buf, lay, mode, inv_k, max_blocks=0):
  del max_blocks                                     # the result depends on the operands alone
  n, a, g = lay['n'], lay['acc'], lay['g']
  l, la, lm = lay['loss'], lay['loss_acc'], lay['loss_mean']
  if mode == FIRST:
    buf[a:a + n] = buf[g:g + n]
    buf[la] = buf[l]
  elif mode == ADD:
    buf[a:a + n] = add32(buf[a:a + n], buf[g:g + n])
    buf[la] = add32(buf[la:la + 1], buf[l:l + 1])[0]
  else:
    buf[g:g + n] = add32(buf[a:a + n], buf[g:g + n])
    s = floats(add32(buf[la:la + 1], buf[l:l + 1]))
    with np.errstate(all='ignore'):
      buf[lm] = bits(s * F32(inv_k))[0]


# ---- cases -------------------------------------------------------------------------------------------------------------------
def _order_triples(rng, count):
  """(a, b, c) for which fl(fl(a+b)+c), fl(a+fl(b+c)) and the fp32 rounding of the fp64 sum are three bit patterns."""
  out = []
  while len(out) < count:
    a, b, c = (rng.standard_normal(3) * 10.0 ** rng.integers(-3, 4, 3)).astype(F32)
    if len(set(order_variants(a, b, c))) == 3:
      out.append((a, b, c))
  return out


def order_variants(a, b, c):
  a, b, c = F32(a), F32(b), F32(c)
  ltr = F32(F32(a + b) + c)
  rtl = F32(a + F32(b + c))
  wide = F32(np.float64(a) + np.float64(b) + np.float64(c))
  return int(bits(ltr)[0]), int(bits(rtl)[0]), int(bits(wide)[0])


def loss_variants(l1, l2, l3, k=3):
  """The mean the kernel computes, the mean by division, the mean rounded once from fp64 -- as bit patterns."""
  s = F32(F32(F32(l1) + F32(l2)) + F32(l3))
  by_mul = F32(s * F32(1.0 / k))
  by_div = F32(s / F32(k))
  wide = F32((np.float64(l1) + np.float64(l2) + np.float64(l3)) / np.float64(k))
  return int(bits(by_mul)[0]), int(bits(by_div)[0]), int(bits(wide)[0])


def _loss_triples(rng, count):
  out = []
  while len(out) < count:
    l = (rng.random(3) * 3.0 + 0.5).astype(F32)
    m, d, w = loss_variants(*l)
    if m != d and m != w:
      out.append(tuple(l))
  return out


def _special_columns(rng):
  """name -> (g1, g2, g3) bit patterns, one column per micro-batch."""
  pz, nz = 0x00000000, 0x80000000
  z = [(a, b, c) for a in (pz, nz) for b in (pz, nz) for c in (pz, nz)]
  tri = _order_triples(rng, 9)
  cols = {
      'signed_zeros': z,
      'subnormal_sum_subnormal': [(0x00000001, 0x00000002, 0x00000004), (0x80000003, 0x00000001, 0x00000001),
                                  (0x00400000, 0x00200000, 0x80100000)],
      'subnormal_sum_normal': [(0x007FFFFF, 0x00000001, 0x00000000), (0x00400000, 0x00400000, 0x00400000),
                               (0x807FFFFF, 0x807FFFFF, 0x00000001)],
      'overflow': [(FLT_MAX, FLT_MAX, 0xFF7FFFFF), (0xFF7FFFFF, 0xFF7FFFFF, FLT_MAX), (FLT_MAX, 0x73000000, 0x73000000)],
      'inf_minus_inf': [(0x7F800000, 0xFF800000, 0x3F800000), (0xFF800000, 0x3F800000, 0x7F800000)],
      'nan': [(0x7FC00000, 0x3F800000, 0x40000000), (0x3F800000, 0x7FC00001, 0x40000000), (0x3F800000, 0x40000000, 0xFFC00000)],
      'order_triples': [tuple(int(bits(x)[0]) for x in t) for t in tri],
  }
  return {k: np.array(v, dtype=U32) for k, v in cols.items()}


def _random_bits(rng, n):
  """Finite, non-zero fp32 of mixed magnitude (so that every addition changes its operand)."""
  x = rng.standard_normal(n) * 10.0 ** rng.integers(-2, 3, n)
  x = np.where(x == 0, 1.0, x).astype(F32)
  return bits(x)


def sizes():
  s = {0, 1, 3, 4, 5, WAVE - 1, WAVE, WAVE + 1, TILE - 1, TILE, TILE + 1}
  for mb in (1, 3):
    s |= {mb * TILE - 1, mb * TILE, mb * TILE + 1}
  s |= {2 * TILE + WAVE + 7}                         # wraps max_blocks = 1, with a vector remainder and a scalar tail
  return sorted(s)


def build_cases(seed=20260101):
  """The list of cases: dicts with 'name', 'n', 'stale' (what acc holds before FIRST), 'g' ([3][n] bit patterns), 'm' (how many
  leading elements hold special columns) and 'loss' (three fp32).  One per size (random data, every special column at its
  start, the last five elements random), one per special column alone at an odd size, and n == 0 with a loss."""
  rng = np.random.default_rng(seed)
  cols = _special_columns(rng)
  losses = _loss_triples(rng, 4)
  every = np.concatenate(list(cols.values()))
  cases = []

  def case(name, n, special):
    g = np.stack([_random_bits(rng, n) for _ in range(3)]) if n else np.zeros((3, 0), dtype=U32)
    m = min(len(special), max(n - 5, 0)) if name.startswith('size') else min(len(special), n)
    if m:
      g[:, :m] = special[:m].T
    return dict(name=name, n=n, m=m, stale=_random_bits(rng, n), g=g, loss=losses[len(cases) % len(losses)])
  for n in sizes():
    cases.append(case('size_%d' % n, n, every))
  for name, col in cols.items():
    reps = np.concatenate([col] * -(-7 // len(col)))
    cases.append(case(name, len(reps) | 1, reps))    # an odd size: the scalar tail sees them too
  c = case('loss_triple', 0, every)                  # n == 0 with a loss still does the loss arithmetic
  c['loss'] = losses[0]
  cases.append(c)
  return cases


def state_before(case, mode):
  """The buffer in front of stage ``mode`` of the case's chain, as the reference leaves it, and its layout."""
  lay = layout(case['n'])
  l = [int(bits(x)[0]) for x in case['loss']]
  buf = make_buffer(lay, case['stale'], case['g'][0], l[0], 0x40A00000, 0x40C00000)   # stale loss_acc 5.0, loss_mean 6.0
  for m in range(mode):
    reference(buf, lay, m, 1.0 / 3)
    n = lay['n']
    buf[lay['g']:lay['g'] + n] = case['g'][m + 1]
    buf[lay['loss']] = l[m + 1]
  return buf, lay


def _written(lay, mode):
  """Index ranges stage ``mode`` writes."""
  n = lay['n']
  dst = lay['g'] if mode == LAST else lay['acc']
  sc = lay['loss_mean'] if mode == LAST else lay['loss_acc']
  return [(dst, dst + n), (sc, sc + 1)]


def compare(got, want, lay, modes):
  """Complaints of ``got`` against ``want``: zero differing bits everywhere; only inside what a stage that ADDS writes may a
  NaN differ in its payload, and must still be a NaN."""
  out = []
  differ = got != want
  nan_ok = np.zeros(len(want), dtype=bool)
  inside = np.zeros(len(want), dtype=bool)
  for mode in modes:
    for b, e in _written(lay, mode):
      inside[b:e] = True
      if mode != FIRST:
        nan_ok[b:e] = True
  differ &= ~(nan_ok & is_nan(want) & is_nan(got))
  if np.any(differ & inside):
    i = int(np.flatnonzero(differ & inside)[0])
    out.append('value: word %d is %08x, expected %08x (%d words differ)' % (i, got[i], want[i], int(np.sum(differ & inside))))
  if np.any(differ & ~inside):
    i = int(np.flatnonzero(differ & ~inside)[0])
    where = 'guard / slack / unwritten operand'
    out.append('untouched: word %d (%s) is %08x, was %08x' % (i, where, got[i], want[i]))
  return out


def check_stage(impl, case, mode, max_blocks=0, inv_k=1.0 / 3):
  before, lay = state_before(case, mode)
  want = before.copy()
  reference(want, lay, mode, inv_k)
  got = before.copy()
  impl(got, lay, mode, inv_k, max_blocks)
  out = compare(got, want, lay, [mode])
  again = before.copy()
  impl(again, lay, mode, inv_k, max_blocks)
  if not np.array_equal(again, got):
    out.append('repeat: a second run from the same state differs')
  return out


def check_chain(impl, case, max_blocks=0, inv_k=1.0 / 3, ref=reference):
  """FIRST, ADD, LAST over the case's three gradients and losses; the end state against the reference's."""
  results = []
  for f in (impl, ref):
    buf, lay = state_before(case, FIRST)
    n = lay['n']
    for m in MODES:
      if m:
        buf[lay['g']:lay['g'] + n] = case['g'][m]
        buf[lay['loss']] = int(bits(case['loss'][m])[0])
      f(buf, lay, m, inv_k, max_blocks)
    results.append(buf)
  return compare(results[0], results[1], lay, [ADD, LAST])
