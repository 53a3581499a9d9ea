"""Edge cases for K2 (prune_regrow.hip) and K3 momentum (optimizer.hip): deterministic, seeded NumPy builders and
the placement helper that carves operands out of one guarded buffer.  No GPU code: tests/test_k23_cases_cpu.py proves on
the CPU that every case has the property it is named for (and that mutant oracles are rejected), and
tests/test_k2_edges_gpu.py / tests/test_k3_edges_gpu.py run the kernels on the same cases.

A K2 case is a dict: name, branch (the kernel branch it is for), mask / w / g fp32 [n], optional noise / mom / mom2,
frac, grow_init ('zeros', 'grad_scale_<d>', 'grad_sign_<d>'), acc_scale.  NaN is excluded everywhere: tf.nn.top_k's
order on NaN is not defined."""
import numpy as np

import adam_ref
from oracle import rigl_oracle as O

F32 = np.float32

# word (32), segment (1024) and chunk (4096) edges of K2, quad (4) edges of K3, one layer of three chunks
SIZES = (1, 2, 3, 4, 5, 31, 32, 33, 1023, 1024, 1025, 4095, 4096, 4097, 8193)
OFFSETS = (0, 1, 2, 3)          # element offsets of fp32 operands from a 256-byte boundary
GUARD = 64                      # guard elements on each side of every operand
SENTINEL = 0xDEADBEEF           # the guards' bit pattern: a finite fp32 (-6.26e18), two non-zero bf16, a dense bitmap word
CHUNK = 4096


# ------------------------------------------------------------------------------------------------------------ placement
class Placement:
  """Operands carved out of ONE byte buffer.  Operand i starts at a 256-byte boundary + GUARD elements + its element
  offset and is followed by at least GUARD elements; everything that is not an operand holds SENTINEL.  `buffer` is the
  host image (upload it, run, download it); `views(buf)` returns the operands of any image of the same layout and
  `guards_intact(buf)` tells whether every byte outside the operands is still the sentinel's."""

  def __init__(self, operands, offset=0, offsets=None):
    """operands: dict name -> array (fp32 / uint32 / uint16, flat).  fp32 operands are placed `offset` elements off the
    boundary (per-name overrides, any dtype, in `offsets`); bitmaps (uint32) and bf16 (uint16) stay aligned."""
    offsets = dict(offsets or {})
    self.spans = {}
    pos = 0
    for name, a in operands.items():
      a = np.ascontiguousarray(a).reshape(-1)
      off = offsets.get(name, offset if a.dtype == np.float32 else 0)
      start = pos + (GUARD + off) * a.itemsize
      self.spans[name] = (start, a.nbytes, a.dtype)
      pos = -(-(start + a.nbytes + GUARD * a.itemsize) // 256) * 256
    self.nbytes = pos
    self.buffer = self.blank()
    self._outside = np.ones(self.nbytes, bool)
    for name, a in operands.items():
      start, nb, _ = self.spans[name]
      self.buffer[start:start + nb] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
      self._outside[start:start + nb] = False

  def blank(self):
    return np.full(self.nbytes // 4, SENTINEL, np.uint32).view(np.uint8).copy()

  def span(self, name):
    """(byte offset, byte length, dtype) of an operand."""
    return self.spans[name]

  def views(self, buf=None):
    buf = self.buffer if buf is None else np.asarray(buf).reshape(-1).view(np.uint8)
    return {name: buf[s:s + nb].view(dt) for name, (s, nb, dt) in self.spans.items()}

  def guards_intact(self, buf=None):
    buf = self.buffer if buf is None else np.asarray(buf).reshape(-1).view(np.uint8)
    return bool(buf.size == self.nbytes and np.array_equal(buf[self._outside], self.blank()[self._outside]))


def pack_bits(mask01):
  """0/1 array -> uint32 bitmap words (bit i of word j = element 32 j + i, tail bits zero)."""
  m = np.asarray(mask01).reshape(-1).astype(np.uint8)
  m = np.concatenate([m, np.zeros((-m.size) % 32, np.uint8)])
  return np.packbits(m, bitorder='little').view('<u4').astype(np.uint32)


def unpack_bits(words, n):
  return np.unpackbits(np.ascontiguousarray(words, np.uint32).view(np.uint8), bitorder='little')[:n].astype(F32)


def bf16_bits(a):
  """bf16 round-to-nearest-even of finite fp32 values, as uint16."""
  u = np.asarray(a, F32).reshape(-1).view(np.uint32).astype(np.uint64)
  return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


# ------------------------------------------------------------------------------------------------------------- K2 cases
def _case(name, branch, mask, w, g, frac, noise=None, mom=None, mom2=None, grow_init='zeros', acc_scale=0.0):
  f = lambda a: None if a is None else np.ascontiguousarray(a, F32).reshape(-1)
  return dict(name=name, branch=branch, mask=f(mask), w=f(w), g=f(g), noise=f(noise), mom=f(mom), mom2=f(mom2),
              frac=float(frac), grow_init=grow_init, acc_scale=float(acc_scale))


def size_case(n, noise=False, slots=0, seed=0):
  """An ordinary layer of n weights quantised to 1/8 (ties at every threshold), half of them active."""
  rs = np.random.RandomState(1000 * seed + n)
  q = lambda a: (np.round(a * 8) / 8).astype(F32)
  mask = (rs.rand(n) < 0.5).astype(F32)
  if n <= 5:
    mask[::2] = 1                                     # tiny layers: something to prune
  w, g = q(rs.randn(n)), q(rs.randn(n) * 2)
  nz = q(rs.randn(n) * 0.25) if noise else None       # negative drop scores on inactive weights included
  mom = rs.randn(n).astype(F32) if slots >= 1 else None
  mom2 = rs.randn(n).astype(F32) if slots >= 2 else None
  return _case('size%d_noise%d_slots%d' % (n, noise, slots), 'load4 tail / unaligned path', mask, w, g, 0.5, nz, mom, mom2,
               acc_scale=0.5 if slots else 0.0)


def mode_cases(n=1500):
  """Gap 3 and 4: degenerate counts and selection modes (k_scan), the fp32 count, the lifted-score overlap."""
  rs = np.random.RandomState(7)
  w, g, mom = rs.randn(n).astype(F32), rs.randn(n).astype(F32), rs.randn(n).astype(F32)
  half = (rs.rand(n) < 0.5).astype(F32)
  ten = np.zeros(n, F32)
  ten[rs.permutation(n)[:10]] = 1
  big = (F32(2.0 ** 26) + 8 * rs.permutation(n)).astype(F32) * np.where(rs.rand(n) < 0.5, -1, 1).astype(F32)
  return [
      _case('n_ones_zero', 'n_ones == 0: k <= 0 in both selections (mode 1)', np.zeros(n), w, g, 0.3, mom=mom),
      _case('dense_mask', 'fully dense mask: every dropped weight is regrown', np.ones(n), w, g, 0.3, mom=mom),
      _case('dense_frac_zero', 'n_keep >= n (mode 2) and n_prune == 0', np.ones(n), w, g, 0.0, mom=mom),
      _case('frac_zero', 'drop_fraction 0: n_prune == 0', half, w, g, 0.0, mom=mom),
      _case('frac_one', 'drop_fraction 1: n_keep == 0', half, w, g, 1.0, mom=mom, acc_scale=0.5),
      _case('frac_tiny', 'drop_fraction 1e-9: n_prune == 0', half, w, g, 1e-9, mom=mom),
      _case('f32_count', 'int32(f32(n_ones) * f32(frac)) != the double product', ten, w, g, 0.7, mom=mom),
      _case('large_distinct_grad', '|g| >= 2^26, distinct: min - 1 == min without an overlap', half, w, big, 0.3, mom=mom),
      _case('overlap', 'constant |g| = 2^27: the kept set ties with the smallest gradient (Assert fires)', half, w,
            np.full(n, 2.0 ** 27), 0.3, mom=mom),
  ]


def data_case(n=4097 + 1024, seed=3, grow_init='grad_scale_1000', acc_scale=1e-10):
  """Gap 5, planted at fixed residues of the index (the style of test_adam_gpu._inputs): subnormal weights, noise,
  gradients and products, +-inf scores, negative drop scores over many magnitudes, underflowing grow values / resets."""
  rs = np.random.RandomState(seed)
  k = np.arange(n)
  mask = (rs.rand(n) < 0.5).astype(F32)
  w = rs.randn(n).astype(F32)
  g = rs.randn(n).astype(F32)
  mom = rs.randn(n).astype(F32)
  sub = (F32(1e-45) * rs.randint(1, 1 << 20, n).astype(F32)).astype(F32)       # distinct subnormals
  # subnormal noise everywhere: with few weights dropped the drop threshold lies among subnormal scores
  noise = ((F32(1e-45) * rs.randint(1, 1 << 20, n).astype(F32)) * np.where(rs.rand(n) < 0.5, -1, 1)).astype(F32)
  sel = k % 7 == 0
  w[sel] = sub[sel] * np.where(k[sel] % 2, -1, 1).astype(F32)                  # subnormal weights, both signs
  sel = k % 7 == 0
  noise[sel] = np.where(k[sel] % 3 == 0, sub[::-1][sel], 0).astype(F32)        # subnormal + subnormal, subnormal + 0
  sel = k % 11 == 1
  noise[sel] = sub[sel] * F32(-1)                                              # subnormal noise (negative on inactive)
  sel = k % 13 == 2
  g[sel] = sub[sel] * np.where(k[sel] % 2, -1, 1).astype(F32)                  # subnormal gradients
  sel = k % 17 == 3
  g[sel] = (rs.randn(sel.sum()) * 1e-36).astype(F32)                           # tiny gradients
  sel = k % 19 == 4
  noise[sel] = np.inf                                                          # +inf drop score
  mask[sel] = 1
  g[sel] = np.where(k[sel] % 2, np.inf, -np.inf).astype(F32)                   # +inf grow score on a kept weight (lifted)
  sel = k % 23 == 5
  noise[sel] = -np.inf                                                         # -inf drop score
  g[sel & (mask != 0)] = 0                                                     # a dropped one may regrow: finite reset
  sel = (k % 5 == 2) & (k % 19 != 4)                                           # negative scores across the radix digits,
  mask[sel] = 0                                                                # on inactive weights
  noise[sel] = -(F32(10.0) ** rs.randint(-38, 30, sel.sum()).astype(F32)).astype(F32)
  sel = k % 29 == 6
  g[sel] = np.where(k[sel] % 2, -0.0, 0.0).astype(F32)                         # +-0 gradients
  return _case('data_edges' if n > 1000 else 'data_edges_n%d' % n, 'subnormals, +-inf, negative scores over the digit boundaries', mask, w, g, 0.1, noise, mom,
               grow_init=grow_init, acc_scale=acc_scale)


def negative_threshold_case(n=3000, seed=4):
  """Every drop score negative (noise below -|w|), spread over many exponents: the three radix digits of the threshold
  are those of a negative key."""
  rs = np.random.RandomState(seed)
  mask = (rs.rand(n) < 0.6).astype(F32)
  w = rs.randn(n).astype(F32)
  noise = -(F32(10.0) ** rs.uniform(1, 12, n)).astype(F32)
  return _case('negative_threshold', 'negative drop scores at the threshold', mask, w, rs.randn(n), 0.3, noise, rs.randn(n))


def grad_sign_zero_case(n=1030, seed=5):
  """grad_sign on +-0 (and the reset g * scale on them): most gradients are signed zeros, so they are grown."""
  rs = np.random.RandomState(seed)
  mask = (rs.rand(n) < 0.5).astype(F32)
  g = np.where(np.arange(n) % 2, -0.0, 0.0).astype(F32)
  some = rs.permutation(n)[:40]
  g[some] = rs.randn(40).astype(F32)
  return _case('grad_sign_zero', 'grad_sign on +-0', mask, rs.randn(n), g, 0.5, mom=rs.randn(n), grow_init='grad_sign_10',
               acc_scale=0.5)


def underflow_case(n=1025, seed=6):
  """Every gradient about 1e-36: the grown weight g / 1000 and the slot reset g * 1e-3 are subnormal products."""
  rs = np.random.RandomState(seed)
  mask = (rs.rand(n) < 0.5).astype(F32)
  g = (rs.randn(n) * 1e-36).astype(F32)
  return _case('underflow', 'grad_scale_d / initial_acc_scale results that underflow', mask, rs.randn(n), g, 0.5,
               mom=rs.randn(n), mom2=rs.randn(n), grow_init='grad_scale_1000', acc_scale=1e-3)


def all_k2_cases():
  return mode_cases() + [data_case(), data_case(n=33, seed=9, grow_init='grad_sign_1000', acc_scale=1e-12),
                         negative_threshold_case(), grad_sign_zero_case(), underflow_case()]


def expected_counts(c):
  """n_ones, n_prune, n_keep as sparse_optimizers_base.py:286-290 forms them (also when the update itself asserts)."""
  n_ones = np.int32(np.sum(c['mask'], dtype=F32))
  n_prune = np.int32(F32(F32(n_ones) * F32(c['frac'])))
  return int(n_ones), int(n_prune), int(n_ones - n_prune)


def oracle_update(c):
  """oracle.rigl_mask_update on a case; None when the reference's Assert(mask1 * mask2 == 0) fires."""
  with np.errstate(all='ignore'):
    try:
      return O.rigl_mask_update(c['mask'], c['w'], c['g'], c['frac'], noise=c['noise'], momentum=c['mom'],
                                grow_init=c['grow_init'], initial_acc_scale=c['acc_scale'])
    except AssertionError:
      return None


def oracle_second_slot(c, r):
  """The second slot after the update: reset exactly like the first (sparse_optimizers_base.py:555-564)."""
  with np.errstate(all='ignore'):
    acc = (c['g'] * F32(c['acc_scale'])).astype(F32)
  return np.where(r['new_connections'].reshape(-1), acc, c['mom2']).astype(F32)


# ---- explicit scores (topk_mask, magnitude prune) ------------------------------------------------------------------
def score_case(n, seed=0):
  """Scores for rigl_topk_mask: quantised (ties), both signs, and a block of +-0 with -0.0 at the LOWER indices, so a
  comparator that puts -0.0 below +0.0 picks other entries; +-inf at fixed residues."""
  rs = np.random.RandomState(77 * seed + n)
  s = (np.round(rs.randn(n) * 4) / 4).astype(F32)
  k = np.arange(n)
  zeros = k % 3 == 0
  s[zeros] = np.where(k[zeros] % 2 == 0, -0.0, 0.0).astype(F32)
  if n >= 32:
    s[k % 31 == 7] = np.inf
    s[k % 37 == 9] = -np.inf
  return s


def zero_straddle_k(s):
  """An n_keep that cuts through the block of +-0 scores (None if there is no such block)."""
  above, zeros = int((s > 0).sum()), int((s == 0).sum())
  return above + (zeros + 1) // 2 if zeros >= 2 else None


def topk_mask_ref(s, k):
  m = np.zeros(np.size(s), F32)
  m[O.topk_order(np.asarray(s, F32).reshape(-1))[:max(int(k), 0)]] = 1
  return m


def explicit_score_cases(n, seed=0):
  """Explicit drop / grow scores (the SET / Static / Momentum path of rigl_prune_regrow) with signed zeros and +-inf: one
  case whose drop selection cuts through the +-0 block (drop_fraction 0, n_keep == zero_straddle_k) and one ordinary one.
  The grow scores have no -inf: min - 1 == min would be the overlap case again."""
  rs = np.random.RandomState(31 * seed + n)
  sd, sg = score_case(n, seed), score_case(n, seed + 1)
  sg[np.isneginf(sg)] = -3.0
  w, g, mom = rs.randn(n).astype(F32), rs.randn(n).astype(F32), rs.randn(n).astype(F32)
  out = []
  for tag, n_ones, frac in (('straddle', zero_straddle_k(sd) or 1, 0.0), ('half', n // 2, 0.5)):
    mask = np.zeros(n, F32)
    mask[rs.permutation(n)[:n_ones]] = 1
    c = _case('explicit_%s_%d' % (tag, n), 'explicit scores, -0.0 == +0.0', mask, w, g, frac, mom=mom, acc_scale=0.5)
    c.update(score_drop=sd, score_grow=sg)
    out.append(c)
  return out


def oracle_update_explicit(c):
  """oracle.get_update on explicit scores (grow_init 'zeros', RigL's slot reset)."""
  with np.errstate(all='ignore'):
    return O.get_update(c['score_drop'], c['score_grow'], c['mask'], c['w'], c['frac'], grow_tensor=np.zeros_like(c['w']),
                        momentum=c['mom'], dense_grad=c['g'], initial_acc_scale=c['acc_scale'])


# -------------------------------------------------------------------------------------------------------- batched table
GRID_CAPS = (1536, 2048, 4096)    # workgroups of k_drop_hist<0>, the refinement passes and k_apply1


def _inside_a_range(c, total, wgs):
  """Is chunk boundary c strictly inside the chunk range [c0, c1) of one of the wgs workgroups (chunk_range)?"""
  b = c * wgs // total
  return any(bb * total // wgs < c < (bb + 1) * total // wgs for bb in (b - 1, b, b + 1) if 0 <= bb < wgs)


def layer_table(seed=11, n_layers=5000):
  """About 5000 layers: mostly one chunk each (1 .. 4096 elements, small ones preferred so the whole table stays at a few
  million elements), a few multi-chunk layers and three zero-length layers (first, near the middle, last).  More than 4096 chunks in
  all, so each capped grid (1536 / 2048 / 4096 workgroups) walks ranges that hold complete layers, several of them, and a
  zero-length entry.  Returns the list of sizes."""
  rs = np.random.RandomState(seed)
  small = np.array([1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 100, 255, 257, 500, 1023, 1024, 1025, 2047, 3000, 4095, 4096])
  p = np.where(small <= 100, 3.0, 1.0)
  sizes = rs.choice(small, n_layers, p=p / p.sum()).astype(np.int64)
  multi = {17: 4097, 900: 8193, 2500: 3 * CHUNK + 5, 2501: 2 * CHUNK, 4000: 40000, n_layers - 2: 4097}
  for i, n in multi.items():
    sizes[i] = n
  sizes[0] = sizes[n_layers - 1] = 0
  for mid in range(n_layers // 2, n_layers - 1):      # the middle one: where every grid has it strictly inside a range
    trial = sizes.copy()
    trial[mid] = 0
    first = np.concatenate([[0], np.cumsum(-(-trial // CHUNK))])
    if sizes[mid] <= CHUNK and all(_inside_a_range(int(first[mid]), int(first[-1]), wgs) for wgs in GRID_CAPS):
      return [int(n) for n in trial]
  raise AssertionError('no middle position for the zero-length layer')


def table_case(sizes, seed=12):
  """One arena per operand for the whole table (layer l occupies [start[l], start[l] + n_l): bases at every alignment);
  bitmaps in a word arena, word-aligned per layer.  Weights and gradients quantised: ties at most thresholds."""
  rs = np.random.RandomState(seed)
  total = int(sum(sizes))
  start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
  words = [(n + 31) // 32 for n in sizes]
  wstart = np.concatenate([[0], np.cumsum(words)]).astype(np.int64)
  dens = rs.uniform(0.05, 1.0, len(sizes))
  mask = np.concatenate([(rs.rand(n) < d).astype(F32) for n, d in zip(sizes, dens)] + [np.zeros(0, F32)])
  q = lambda a: (np.round(a * 8) / 8).astype(F32)
  return dict(sizes=list(sizes), start=start, wstart=wstart, total=total, mask=mask, w=q(rs.randn(total)),
              g=q(rs.randn(total) * 2), mom=rs.randn(total).astype(F32), frac=0.3, acc_scale=0.5,
              score=q(rs.randn(total)), n_keep=[int(rs.randint(0, n + 1)) for n in sizes],
              mag_k=[int(rs.randint(1, n + 1)) if n else 0 for n in sizes])


def table_layer(t, l):
  """Layer l of a table as a K2 case."""
  a, b = int(t['start'][l]), int(t['start'][l + 1])
  return _case('table[%d]' % l, 'layer crossing', t['mask'][a:b], t['w'][a:b], t['g'][a:b], t['frac'], mom=t['mom'][a:b],
               acc_scale=t['acc_scale'])


# ------------------------------------------------------------------------------------------------------------- K3 cases
def momentum_inputs(n, seed=0):
  """w, g, a and the mask for the momentum kernel: test_adam_gpu._inputs' plants (zero, huge and tiny values, a subnormal
  slot) plus +-0.0 in g, a and w at masked-on and masked-off positions (mask = index parity inside the +-0 plants, so both
  kinds occur for every sign combination)."""
  rs = np.random.RandomState(500 + seed + n)
  w = rs.randn(n).astype(F32)
  g = rs.randn(n).astype(F32)
  a = (rs.randn(n) * 0.1).astype(F32)
  mask = (rs.rand(n) < 0.4).astype(F32)
  k = np.arange(n)
  g[k % 7 == 0] = 0
  g[k % 11 == 2] *= F32(1e18)
  w[k % 13 == 3] *= F32(1e20)
  g[k % 17 == 4] *= F32(1e-30)
  a[k % 19 == 5] = F32(1e-40)        # subnormal
  a[k % 23 == 6] = F32(3e25)
  # signed zeros: the 16 sign / zero combinations of (g, a, w), each at a masked-on and a masked-off position,
  # a zero weight with either sign
  z = k % 3 == 1
  c = (k // 3) % 64
  sg = np.where(c & 1, -1.0, 1.0).astype(F32)
  g[z] = np.where(c[z] & 2, F32(0) * sg[z], np.abs(g[z]) * sg[z] + sg[z])          # +-0 or +-(nonzero)
  a[z] = np.where(c[z] & 4, -0.0, 0.0).astype(F32)
  w[z] = np.where(c[z] & 8, np.where(c[z] & 32, -0.0, 0.0), -np.abs(w[z]) - 1).astype(F32)
  mask[z] = (c[z] >> 4) & 1
  return w, g, a, mask


# (lr, mu, wd, grad_scale, nesterov): lr = 0, mu of 0 and 1, wd of 0 and non-zero, grad_scale of 1 and 0.125
MOMENTUM_GRID = [
    (0.1, 0.9, 0.0, 1.0, True),
    (0.1, 0.9, 1e-4, 1.0, True),
    (0.1, 0.9, 1e-4, 0.125, False),
    (0.0, 0.9, 1e-4, 1.0, True),
    (0.05, 0.0, 0.0, 0.125, True),
    (0.05, 1.0, 5e-4, 1.0, False),
    (0.0, 0.0, 0.0, 1.0, False),
]


unified_masked_grad = adam_ref.masked_grad     # the one masked gradient: oracle.masked_grad on grad_scale * dense


def momentum_ref(w, g, a, mask, lr, mu, wd, grad_scale, nesterov, has_mom=True):
  """(w, a, bf16 shadow bits) after one step, by oracle.masked_grad + momentum_apply / sgd_apply."""
  with np.errstate(all='ignore'):
    gv = unified_masked_grad(g, mask, w, wd, grad_scale)
    if has_mom:
      w1, a1 = O.momentum_apply(w, a, gv, lr, mu, nesterov=nesterov)
    else:
      w1, a1 = O.sgd_apply(w, gv, lr), None
  sh = bf16_bits(w1)
  if mask is not None:
    sh = np.where(np.asarray(mask) != 0, sh, 0).astype(np.uint16)
  return w1, a1, sh
