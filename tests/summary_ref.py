"""NumPy reference of the training-summary pass (rigl_summary_step) and the case set the GPU test runs -- TEST
INFRASTRUCTURE, never imported by the product.

Per element the gradient is ``oracle.masked_grad`` on the scaled gradient with K3's rule for a masked-off element (the signed
zero of the scaled gradient, also where it is not finite); the sums are ``math.fsum`` over fp64 terms.  Squares and absolute
values of fp32 numbers are exact in fp64, so a reference sum is the exactly rounded true value, and a sum of n such
non-negative terms accumulated in fp64 in ANY order stays within n * 2^-53 * S of it to first order: the tests allow
``2 * n * 2^-53 * S_ref`` (``bound``).

``entry_sums(..., mutant=NAME)`` computes what a plausible wrong kernel would: tests/test_summary_ref_cpu.py shows that every
mutant is rejected by at least one case of ``tables()``, i.e. that the case set can tell them apart.
"""
import math

import numpy as np

from oracle import rigl_oracle as O

F32 = np.float32
CHUNK = 8192                      # RIGL_SUMMARY_CHUNK
ALIGN = 64                        # elements between entry starts: the arenas' alignment (rigl_amd.variables.ALIGN)
FLOAT_FIELDS = ('sumsq_g', 'sumsq_w', 'l1_w')
COUNT_FIELDS = ('nz_w', 'mask_ones', 'nonfinite_g')
MUTANTS = ('mask_ignored', 'decay_dropped', 'scale_after_sum', 'fma_contracted', 'neg_zero_nonzero', 'subnormals_flushed',
           'padding_read', 'masked_off_inf_counted', 'fp32_accumulation', 'tail_bits_counted')


def bound(n_terms, s_ref):
  return 2.0 * n_terms * 2.0 ** -53 * s_ref


def unpack_bits(words, n):
  """uint32 words -> 0/1 fp32 [n] (bit i & 31 of word i >> 5)."""
  w = np.ascontiguousarray(words, dtype=np.uint32)
  return np.unpackbits(w.view(np.uint8), bitorder='little')[:n].astype(F32)


def masked_gradient(w, g, m01, weight_decay, grad_scale):
  """gq = f32(f32(m * f32(grad_scale * g)) + f32(weight_decay * w)), masked-off non-finite gradients as signed zeros."""
  with np.errstate(all='ignore'):
    gs = (F32(grad_scale) * g.astype(F32)).astype(F32)
    gs = np.where(m01 != 0, gs, np.copysign(F32(0), gs)).astype(F32)
    return O.masked_grad(gs, m01, w, weight_decay)


def _fsum(x):
  x = np.asarray(x, dtype=np.float64)
  if np.isnan(x).any():
    return float('nan')
  if np.isinf(x).any():
    return float('inf')                               # the terms are non-negative
  return math.fsum(x.tolist())


def entry_sums(e, grad_scale, mutant=None):
  """The six outputs of one entry.  ``e``: dict with n, w_buf / g_buf (fp32, at least n elements: what lies behind n is the
  arena's padding), bits (uint32 words, or None), weight_decay, apply_mask."""
  n = e['n'] + (1 if mutant == 'padding_read' else 0)
  w, g = e['w_buf'][:n].astype(F32), e['g_buf'][:n].astype(F32)
  bit = unpack_bits(e['bits'], n) if e['bits'] is not None else np.ones(n, F32)
  m = bit if (e['apply_mask'] and mutant != 'mask_ignored') else np.ones(n, F32)
  wd = 0.0 if mutant == 'decay_dropped' else e['weight_decay']
  with np.errstate(all='ignore'):
    if mutant == 'scale_after_sum':
      gq = (F32(grad_scale) * O.masked_grad(np.where(m != 0, g, np.copysign(F32(0), g)).astype(F32), m, w, wd)).astype(F32)
    elif mutant == 'fma_contracted':
      gs = (F32(grad_scale) * g).astype(F32)
      gs = np.where(m != 0, gs, np.copysign(F32(0), gs)).astype(np.float64)
      gq = (gs + np.float64(F32(wd)) * w.astype(np.float64)).astype(F32)   # one rounding: the product is exact in fp64
    elif mutant == 'masked_off_inf_counted':
      gs = (F32(grad_scale) * g).astype(F32)
      gq = O.masked_grad(gs, m, w, wd)                # 0 * inf = NaN
    else:
      gq = masked_gradient(w, g, m, wd, grad_scale)
    if mutant == 'subnormals_flushed':
      tiny = np.abs(w) < F32(2.0 ** -126)
      w = np.where(tiny, np.copysign(F32(0), w), w).astype(F32)
    gd, wdbl = gq.astype(np.float64), w.astype(np.float64)
    terms = {'sumsq_g': gd * gd, 'sumsq_w': wdbl * wdbl, 'l1_w': np.abs(wdbl)}
    out = {}
    for k, t in terms.items():
      if mutant == 'fp32_accumulation':
        out[k] = float(np.cumsum(t.astype(F32), dtype=F32)[-1]) if n else 0.0   # (cumsum accumulates sequentially, in fp32)
      else:
        out[k] = _fsum(t)
  if mutant == 'neg_zero_nonzero':
    out['nz_w'] = int(np.count_nonzero(w.view(np.uint32)))
  else:
    out['nz_w'] = int(np.count_nonzero(w != 0))
  if e['bits'] is None:
    out['mask_ones'] = int(n)
  elif mutant == 'tail_bits_counted':
    words = np.ascontiguousarray(e['bits'][:(n + 31) // 32], dtype=np.uint32)
    out['mask_ones'] = int(np.unpackbits(words.view(np.uint8)).sum())
  else:
    out['mask_ones'] = int(bit.sum())
  out['nonfinite_g'] = int(np.count_nonzero(~np.isfinite(gq)))
  return out


def table_sums(table, mutant=None):
  """({field: [per entry]}, {field: total}) of a table of ``tables()``.  A floating-point total is the fsum of the per-entry
  references: each of those is exactly rounded, so the total is within 2 * 2^-53 relative of the true one -- far inside
  ``bound`` with the table's element count, which is what the tests allow a total."""
  per = [entry_sums(e, table['grad_scale'], mutant) for e in table['entries']]
  ent = {k: [p[k] for p in per] for k in FLOAT_FIELDS + COUNT_FIELDS}
  tot = {k: _fsum(ent[k]) for k in FLOAT_FIELDS}
  tot.update({k: int(sum(ent[k])) for k in COUNT_FIELDS})
  return ent, tot


def same_class(a, b):
  """Both NaN, both +inf, or both finite."""
  if math.isnan(a) or math.isnan(b):
    return math.isnan(a) and math.isnan(b)
  if math.isinf(a) or math.isinf(b):
    return a == b
  return True


def float_ok(got, ref, n_terms):
  """A floating-point output against its reference: the same class, and within ``bound`` where finite."""
  if not same_class(got, ref):
    return False
  if not math.isfinite(ref):
    return True
  return abs(got - ref) <= bound(n_terms, ref)


def differs(a, b, n_list):
  """True where the outputs ``a`` of a candidate (per-entry dict of lists) would FAIL the GPU test's assertions against b."""
  for k in COUNT_FIELDS:
    if list(a[k]) != list(b[k]):
      return True
  for k in FLOAT_FIELDS:
    for x, y, n in zip(a[k], b[k], n_list):
      if not float_ok(x, y, max(n, 1)):
        return True
  return False


# ---- the case set ---------------------------------------------------------------------------------------------------------
EDGE_SIZES = (1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)
MASK_KINDS = ('ones', 'zeros', 'null', 'last', 'ragged')


def _mask_words(kind, n, rs):
  """ceil(n / 32) words; the bits at positions >= n of the last word are SET (a kernel must not count them)."""
  if kind == 'null':
    return None
  if kind == 'ones':
    m = np.ones(n, np.uint8)
  elif kind == 'zeros':
    m = np.zeros(n, np.uint8)
  elif kind == 'last':
    m = np.zeros(n, np.uint8)
    m[-1:] = 1
  else:
    m = (rs.rand(n) < 0.3).astype(np.uint8)
  nw = (n + 31) // 32
  padded = np.ones(nw * 32, np.uint8)
  padded[:n] = m
  return np.packbits(padded, bitorder='little').view(np.uint32).copy()


def _pack(specs, grad_scale, rs, name):
  """Lays the entries out as the arenas do: starts on ALIGN elements, the padding filled with finite garbage (w 7, g 11, mask
  words all ones), one ALIGN of it behind the last entry."""
  total = sum(-(-s['n'] // ALIGN) * ALIGN for s in specs) + ALIGN
  W = np.full(total, 7.0, F32)
  G = np.full(total, 11.0, F32)
  B = np.full(total // 32, 0xFFFFFFFF, np.uint32)
  off, entries = 0, []
  for s in specs:
    n = s['n']
    W[off:off + n] = s['w']
    G[off:off + n] = s['g']
    bits = None
    if s['bits'] is not None:
      B[off // 32:off // 32 + len(s['bits'])] = s['bits']
      bits = B[off // 32:]
    entries.append({'n': n, 'offset': off, 'w_buf': W[off:], 'g_buf': G[off:], 'bits': bits, 'has_mask': s['bits'] is not None,
                    'weight_decay': s['weight_decay'], 'apply_mask': s['apply_mask']})
    off += -(-n // ALIGN) * ALIGN
  return {'name': name, 'grad_scale': grad_scale, 'entries': entries, 'W': W, 'G': G, 'B': B}


def _data(n, rs, specials=True):
  w = rs.randn(n).astype(F32)
  g = rs.randn(n).astype(F32)
  if specials and n >= 4:
    idx = rs.permutation(n)
    w[idx[0]] = F32(0.0)
    w[idx[1]] = F32(-0.0)
    w[idx[2]] = F32(1e-42)                            # subnormal
    w[idx[3]] = F32(-3e-45)
    g[idx[1]] = F32(-0.0)
  elif specials:
    w[0] = F32(-0.0) if n == 1 else F32(1e-42)
  return w, g


_WDS = (0.0, 1e-4, 5e-4)


def tables():
  """The GPU case set: a list of tables (see _pack).  At most 1 M elements in all."""
  rs = np.random.RandomState(1234)
  out = []
  # (1) the edge sizes, every mask kind on every size class, zero-length entries in between
  specs = []
  for i, n in enumerate(EDGE_SIZES):
    for j in range(2 if n < CHUNK - 1 else 1):
      kind = MASK_KINDS[(i + 3 * j) % len(MASK_KINDS)] if n < CHUNK - 1 else ('ragged', 'last', 'ragged', 'ones')[i % 4]
      w, g = _data(n, rs)
      specs.append({'n': n, 'w': w, 'g': g, 'bits': _mask_words(kind, n, rs), 'weight_decay': _WDS[(i + j) % 3], 'apply_mask': 1})
    specs.append({'n': 0, 'w': np.zeros(0, F32), 'g': np.zeros(0, F32), 'bits': None, 'weight_decay': 0.0, 'apply_mask': 1})
  n = CHUNK + 37                                      # DNW's form: a bitmap that is counted and not applied, no decay
  w, g = _data(n, rs)
  specs.append({'n': n, 'w': w, 'g': g, 'bits': _mask_words('ragged', n, rs), 'weight_decay': 0.0, 'apply_mask': 0})
  out.append(_pack(specs, 0.3, rs, 'edges'))
  # (2) 300 small entries: more than four by-value batches
  specs = []
  for i in range(300):
    n = 1 + (i * 7) % 50
    w, g = _data(n, rs)
    specs.append({'n': n, 'w': w, 'g': g, 'bits': _mask_words(MASK_KINDS[i % 5], n, rs), 'weight_decay': _WDS[i % 3],
                  'apply_mask': 1})
  out.append(_pack(specs, 1.0, rs, 'small300'))
  # (3) non-finite gradients at masked-on and masked-off positions, non-finite weights
  specs = []
  for k, (val, where) in enumerate([(np.inf, 'off'), (-np.inf, 'off'), (np.nan, 'off'), (np.inf, 'on'), (-np.inf, 'on'),
                                    (np.nan, 'on'), (np.inf, 'null'), (np.nan, 'null'), ('w_inf', 'null'), ('w_nan', 'null'),
                                    ('inf_and_nan', 'on')]):
    n = 100 + k
    w, g = _data(n, rs, specials=False)
    m = np.zeros(n, np.uint8)
    m[::3] = 1
    pos_on, pos_off = 33, 34                          # 33 % 3 == 0: on;  34: off
    bits = None
    if where != 'null':
      nw = (n + 31) // 32
      padded = np.ones(nw * 32, np.uint8)
      padded[:n] = m
      bits = np.packbits(padded, bitorder='little').view(np.uint32).copy()
    if val == 'w_inf':
      w[5] = np.inf
    elif val == 'w_nan':
      w[5] = np.nan
    elif val == 'inf_and_nan':
      g[pos_on] = np.inf
      g[pos_on + 3] = np.nan
      g[pos_off] = np.inf
    else:
      g[pos_off if where == 'off' else pos_on] = val
    specs.append({'n': n, 'w': w, 'g': g, 'bits': bits, 'weight_decay': _WDS[k % 3], 'apply_mask': 1})
  out.append(_pack(specs, 0.5, rs, 'nonfinite'))
  # (4) entries long enough for the finalize's wave-per-entry path (more than 8 chunks) and for more than one chunk per lane there
  specs = []
  for n, kind, wd in ((9 * CHUNK + 5, 'ragged', 1e-4), (65 * CHUNK + 1, 'ragged', 5e-4)):
    w, g = _data(n, rs)
    specs.append({'n': n, 'w': w, 'g': g, 'bits': _mask_words(kind, n, rs), 'weight_decay': wd, 'apply_mask': 1})
  out.append(_pack(specs, 0.3, rs, 'long'))
  assert sum(t['W'].size for t in out) <= 1 << 20
  return out
