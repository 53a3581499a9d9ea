"""NumPy reference of rigl_state_gather / rigl_state_scatter (include/rigl_hip.h) and the seeded cases its tests share --
TEST INFRASTRUCTURE, never imported by the product.

  offsets(sizes)        region r's byte offset in the packed image: the running sum of the earlier sizes, each rounded up to 256
  digest(words)         (s1, s2) as Python ints: sum w_i and sum (i + 1) * w_i mod 2^64, from NumPy uint64 arithmetic
  image(regions)        the packed image (zero padding) and the digests of a list of uint32 arrays
  CASES / build(name)   the case set; a Case carves its regions out of ONE sentinel-filled buffer, each between guards and at a
                        chosen word offset off 16-byte alignment, so the same bytes serve the NumPy models and the device
"""
import numpy as np

ALIGN = 256                  # RIGL_STATE_ALIGN
CHUNK = 16384                # RIGL_STATE_CHUNK (words): one workgroup moves a chunk at a time
TILE = 4096                  # words a workgroup moves per loop iteration (256 lanes x 4 x 16 B)
ROW = 1024                   # words of one 16-byte access per lane over the workgroup
BATCH = 64                   # RIGL_STATE_BATCH: regions per launch
SENTINEL = 0xA5              # guard bytes (tests/wsguard.py's)
GUARD = 1 << 20              # bytes of guard around a region on the device
MASK64 = (1 << 64) - 1


def pad(n):
  return -(-int(n) // ALIGN) * ALIGN


def offsets(sizes):
  """([byte offset of every region], total bytes) for region byte sizes."""
  out, off = [], 0
  for n in sizes:
    out.append(off)
    off += pad(n)
  return out, off


def digest(words):
  w = np.ascontiguousarray(words).view(np.uint32).reshape(-1).astype(np.uint64)
  with np.errstate(over='ignore'):
    s1 = w.sum(dtype=np.uint64)
    s2 = (w * np.arange(1, w.size + 1, dtype=np.uint64)).sum(dtype=np.uint64)
  return int(s1), int(s2)


def digest_bigint(words):
  """The definition, in Python's unbounded integers."""
  s1 = s2 = 0
  for i, w in enumerate(np.asarray(words).view(np.uint32).reshape(-1).tolist()):
    s1 += w
    s2 += (i + 1) * w
  return s1 & MASK64, s2 & MASK64


def image(regions):
  """(packed uint8 image with zero padding, [(s1, s2)]) of a list of uint32 arrays."""
  offs, total = offsets([4 * r.size for r in regions])
  packed = np.zeros(total, dtype=np.uint8)
  for r, o in zip(regions, offs):
    packed[o:o + 4 * r.size] = r.view(np.uint8)
  return packed, [digest(r) for r in regions]


def random_words(rng, n):
  """Random bit patterns with NaN payloads, -0.0, +0.0, subnormals and infinities sprinkled in."""
  w = rng.randint(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
  special = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0xFF800000, 0x7F800000, 0x80000000, 0x00000000, 0x00000001,
                      0x807FFFFF, 0x00400000], dtype=np.uint32)
  if n:
    k = max(1, n // 7)
    at = rng.randint(0, n, size=k)
    w[at] = special[rng.randint(0, special.size, size=k)]
  return w


class Case:
  """``words``: the size of every region in words; ``shift``: its pointer's word offset (0..3) off 16-byte alignment;
  ``fill``: None for random_words, or the word every region holds."""

  def __init__(self, name, words, shift=None, fill=None, seed=0):
    self.name, self.words, self.fill, self.seed = name, [int(w) for w in words], fill, seed
    self.shift = [int(s) for s in (shift if shift is not None else [i % 4 for i in range(len(words))])]
    assert len(self.shift) == len(self.words) and all(0 <= s < 4 for s in self.shift)

  def regions(self):
    rng = np.random.RandomState(1234 + self.seed)
    if self.fill is not None:
      return [np.full(w, self.fill, dtype=np.uint32) for w in self.words]
    return [random_words(rng, w) for w in self.words]

  def layout(self, guard=GUARD):
    """(bytes of the carved buffer, [(byte offset, bytes) of every region]): every region between guards of ``guard`` bytes (a
    multiple of 16), at its shift off a 16-byte boundary; the buffer's base is taken as 256-byte aligned."""
    assert guard % 16 == 0 and guard >= 16
    spans, off = [], 0
    for w, s in zip(self.words, self.shift):
      off += guard
      spans.append((off + 4 * s, 4 * w))
      off += -(-(4 * s + 4 * w) // 16) * 16
    return off + guard, spans

  def carve(self, guard=GUARD, regions=None):
    """One sentinel-filled uint8 buffer laid out by ``layout``; returns (buffer, spans).  ``regions``: the data, or None for
    sentinel-filled regions (a scatter's destination)."""
    total, spans = self.layout(guard)
    buf = np.full(total, SENTINEL, dtype=np.uint8)
    if regions is not None:
      for (o, n), r in zip(spans, regions):
        buf[o:o + n] = r.view(np.uint8)
    return buf, spans

  @staticmethod
  def outside_intact(buf, spans):
    """True where every byte of ``buf`` outside the spans is still the sentinel."""
    keep = np.ones(buf.size, dtype=bool)
    for o, n in spans:
      keep[o:o + n] = False
    return bool((buf[keep] == SENTINEL).all())


def _table(n, seed):
  """n regions of 0..40 words, zero-length at the first, the last and the 64th place."""
  rng = np.random.RandomState(77 + seed)
  words = rng.randint(1, 41, size=n).tolist()
  for at in (0, n - 1, BATCH - 1):
    if at < n:
      words[at] = 0
  return words


def _edges():
  out = []
  for edge in (ROW, TILE, CHUNK, 2 * CHUNK):
    out += [edge - 1, edge, edge + 1]
  return out


CASES = {c.name: c for c in [
    Case('small', [0, 1, 3, 4, 5, 63, 64, 65]),
    Case('small_shifted', [0, 1, 3, 4, 5, 63, 64, 65], shift=[3, 2, 1, 3, 2, 1, 3, 2]),
    Case('edges', _edges()),
    Case('edges_aligned', _edges(), shift=[0] * 12),
    Case('table_1', [7], shift=[1]),
    Case('table_1_empty', [0], shift=[2]),
    Case('table_64', _table(64, 0)),
    Case('table_65', _table(65, 1)),
    Case('table_129', _table(129, 2)),
    Case('long', [1048577], shift=[0]),
    Case('wrap', [131072], shift=[0], fill=0xFFFFFFFF),
]}
WRAP_LEAST = 92682           # the least count of 0xFFFFFFFF words whose s2 exceeds 2^64


def build(name):
  return CASES[name]
