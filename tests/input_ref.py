"""TEST INFRASTRUCTURE: the NumPy reference of the device CIFAR input pipeline (rigl_cifar_batch, include/rigl_hip.h), written
from the header's semantics: integer-sum standardization in np.float32 operations, the mirror / crop / flip index map, the
draws and round keys from the oracle's stateless stream (oracle/tf_random.py), the Feistel sample order, eval mode.  Never
imported by the product.

  standardize(img)                 uint8 [32, 32, 3] -> float32 [32, 32, 3]
  bf16_bits(y32)                   float32 -> uint16 patterns, round to nearest even
  source(p) / index_map(oy, ox, f) padded coordinate -> source; (rows [32], cols [32]) of one crop
  draws(batch, seed0, step)        oy, ox, flip per image of the batch
  order(n, seed0, epoch, p)        pi_epoch(p)
  train_indices / eval_indices     dataset index of every image of a batch
  batch(...)                       the whole call: (bit patterns [batch, 32, 32, 3], labels, indices, valid count)
  guarded / assert_same            sentinel bands around an output, and the comparison the tests use
"""
import numpy as np
import torch

from oracle import tf_random as TR

SIDE, CH, PAD = 32, 3, 4
N_PIX = SIDE * SIDE * CH                  # 3072
FEISTEL_MUL, EPOCH_SALT, ROUNDS = 0x9E3779B1, 0x5eed, 6
SENTINEL = 0xA5                           # every guard byte; as bf16 0xA5A5 / fp32 0xA5A5A5A5, as int32 a value no label or index takes
GUARD_BYTES = 4096
BF16, FP32 = 0, 1
TORCH_DTYPES = {BF16: torch.bfloat16, FP32: torch.float32}


# ---- standardization ---------------------------------------------------------------------------------------------------
def standardize(img, floor=True):
  """(float)(n x - S1) * (1.0f / max(sqrtf((float)D), sqrtf(3072.f))), D = n S2 - S1^2, every operation one fp32 rounding.
  ``floor=False`` is a mutant (no stddev floor) for the CPU tests."""
  x = np.asarray(img, dtype=np.uint8).astype(np.int64)
  assert x.shape == (SIDE, SIDE, CH)
  s1, s2 = int(x.sum()), int((x * x).sum())
  d = np.array([N_PIX * s2 - s1 * s1], dtype=np.int64).astype(np.float32)[0]          # int64 -> fp32, RNE
  den = np.sqrt(d, dtype=np.float32)
  if floor:
    den = np.maximum(den, np.sqrt(np.float32(N_PIX), dtype=np.float32))
  with np.errstate(divide='ignore', invalid='ignore'):
    inv = np.float32(1.0) / np.float32(den)
    return ((N_PIX * x - s1).astype(np.float32) * inv).astype(np.float32)


def bf16_bits(y32, mode='rne'):
  """fp32 -> bf16 patterns (uint16) by integer arithmetic on the fp32 pattern; 'trunc' is a mutant."""
  u = np.ascontiguousarray(y32, dtype=np.float32).view(np.uint32).astype(np.uint64)
  if mode == 'rne':
    u = u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))
  return (u >> np.uint64(16)).astype(np.uint16)


def out_bits(y32, dtype):
  """The stored bit patterns: uint16 for bf16, uint32 for fp32."""
  return bf16_bits(y32) if dtype == BF16 else np.ascontiguousarray(y32, dtype=np.float32).view(np.uint32).copy()


# ---- mirror pad, crop, flip ----------------------------------------------------------------------------------------------
def source(p):
  """Padded coordinate 0..39 -> source coordinate 0..31 (the edge pixel is repeated: 3,2,1,0 | 0..31 | 31,30,29,28)."""
  p = np.asarray(p)
  return np.where(p < PAD, PAD - 1 - p, np.where(p < PAD + SIDE, p - PAD, 2 * SIDE + PAD - 1 - p))


def index_map(oy, ox, flip):
  """(rows, cols): out[r, c] = img[rows[r], cols[c]] -- the crop at (oy, ox) of the padded image, then the flip."""
  r = np.arange(SIDE)
  c = SIDE - 1 - r if flip else r
  return source(r + int(oy)), source(c + int(ox))


def augment(img, oy, ox, flip):
  rows, cols = index_map(oy, ox, flip)
  return img[rows][:, cols]


# ---- draws and sample order ----------------------------------------------------------------------------------------------
def _i32(v):
  v = int(v) & 0xFFFFFFFF
  return v - (1 << 32) if v >= 1 << 31 else v


def draws(batch, seed0, step):
  """(oy, ox, flip) [batch] each: image i takes words 4i .. 4i+2 of stateless_u32(4 batch, seed pair [seed0, step])."""
  s0, s1 = TR.tf_seed_pair(0, int(seed0), int(step))
  w = TR.stateless_u32(4 * int(batch), s0, s1).reshape(-1, 4)
  u = ((np.uint32(127) << np.uint32(23)) | (w[:, 2] & np.uint32(0x7FFFFF))).view(np.float32) - np.float32(1.0)   # Uint32ToFloat
  return (w[:, 0] % 9).astype(np.int64), (w[:, 1] % 9).astype(np.int64), u < np.float32(0.5)


# The seed of the GPU tests' train case (N = 37, batch 8, steps 0..9): the smallest positive seed0 whose 80 draws hold every
# corner offset (oy, ox in {0, 8}) with and without flip and the centre (4, 4) unflipped -- found by a scan of draws() on the
# CPU; about one seed in 5 000 qualifies.  The tests assert the coverage before they compare anything.
TRAIN_SEED = 3590


def corner_coverage_missing(batch_size, seed0, steps):
  """The (oy, ox, flip) outcomes among the corners (both flips) and the unflipped centre that the draws never produce."""
  seen = set()
  for s in steps:
    oy, ox, flip = draws(batch_size, seed0, s)
    seen |= set(zip(oy.tolist(), ox.tolist(), [bool(f) for f in flip]))
  need = [(a, b, f) for a in (0, 8) for b in (0, 8) for f in (False, True)] + [(PAD, PAD, False)]
  return [n for n in need if n not in seen]


def half_bits(n):
  return max(1, (int(n - 1).bit_length() + 1) // 2)


def order(n, seed0, epoch, p):
  """pi_epoch(p) for an array of positions p in [0, n): 6-round balanced Feistel over 2h bits, cycle-walked into [0, n)."""
  h = half_bits(n)
  m = (1 << h) - 1
  s0, s1 = TR.tf_seed_pair(0, _i32(seed0) ^ EPOCH_SALT, int(epoch))
  k = TR.stateless_u32(8, s0, s1)[:ROUNDS]

  def enc(v):                                            # uint32 arithmetic: the product wraps mod 2^32
    L, R = (v >> np.uint32(h)) & np.uint32(m), v & np.uint32(m)
    for r in range(ROUNDS):
      f = ((R ^ k[r]) * np.uint32(FEISTEL_MUL)) >> np.uint32(32 - h)
      L, R = R, L ^ f
    return (L << np.uint32(h)) | R

  out = enc(np.array(p, dtype=np.uint32, ndmin=1))
  while True:
    bad = out >= n
    if not bad.any():
      return out.astype(np.int64)
    out[bad] = enc(out[bad])


def steps_per_epoch(n, batch, n_shards=1):
  return int(n) // (int(batch) * int(n_shards))


def train_indices(n, batch, seed0, step, shard=0, n_shards=1):
  """Dataset index of every image of the batch at ``step`` (any int: taken mod 2^32, as the kernel reads the counter)."""
  spe = steps_per_epoch(n, batch, n_shards)
  s = int(step) & 0xFFFFFFFF
  p = (s % spe) * batch * n_shards + shard * batch + np.arange(batch, dtype=np.int64)
  return order(n, seed0, s // spe, p)


def eval_indices(n, batch, b, shard=0, n_shards=1):
  """(indices [valid], valid): the images of eval batch ``b`` that exist."""
  idx = ((int(b) & 0xFFFFFFFF) * n_shards + shard) * batch + np.arange(batch, dtype=np.int64)
  idx = idx[idx < n]
  return idx, int(idx.size)


# ---- the whole call ------------------------------------------------------------------------------------------------------
def batch(images, labels, batch_size, step, dtype, train=True, seed0=0, shard=0, n_shards=1):
  """(bits [valid, 32, 32, 3] uint16 / uint32, labels [valid] int32, indices [valid] int32, valid).  Train: valid == batch."""
  n = images.shape[0]
  if train:
    idx = train_indices(n, batch_size, seed0, step, shard, n_shards)
    oy, ox, flip = draws(batch_size, seed0, _i32(step))
  else:
    idx, _ = eval_indices(n, batch_size, step, shard, n_shards)
    oy, ox, flip = [PAD] * len(idx), [PAD] * len(idx), [False] * len(idx)
  out = np.empty((len(idx), SIDE, SIDE, CH), dtype=np.uint16 if dtype == BF16 else np.uint32)
  for i, j in enumerate(idx):
    out[i] = out_bits(augment(standardize(images[j]), oy[i], ox[i], flip[i]), dtype)
  return out, labels[idx].astype(np.int32), idx.astype(np.int32), len(idx)


# ---- datasets ------------------------------------------------------------------------------------------------------------
def edge_images():
  """The seven images the standardization is pinned on: name -> uint8 [32, 32, 3]."""
  rng = np.random.RandomState(0)
  e = {'random': rng.randint(0, 256, (SIDE, SIDE, CH)), 'zeros': np.zeros((SIDE, SIDE, CH), int),
       'all255': np.full((SIDE, SIDE, CH), 255), 'one_in_zeros': np.zeros((SIDE, SIDE, CH), int),
       'one254_in_255': np.full((SIDE, SIDE, CH), 255), 'two_level': rng.randint(127, 129, (SIDE, SIDE, CH)),
       'half': np.concatenate([np.zeros((16, SIDE, CH), int), np.full((16, SIDE, CH), 255)])}
  e['one_in_zeros'][5, 7, 1] = 1
  e['one254_in_255'][0, 0, 0] = 254
  return {k: v.astype(np.uint8) for k, v in e.items()}


def planted_indices(n):
  """Where dataset() puts the seven edge images: the first seven positions of epoch 0's order under TRAIN_SEED, so the train
  case (whatever its batch size) reads every one of them in its first steps."""
  return order(n, TRAIN_SEED, 0, np.arange(7)).tolist()


def dataset(n, seed=0, plant=True):
  """(images uint8 [n, 32, 32, 3], labels int32 [n]): random bytes, with the seven edge images at planted_indices(n) (n >= 7)."""
  rng = np.random.RandomState(1000 + seed)
  images = rng.randint(0, 256, (n, SIDE, SIDE, CH)).astype(np.uint8)
  labels = rng.randint(0, 10, n).astype(np.int32)
  if plant and n >= 7:
    for i, img in zip(planted_indices(n), edge_images().values()):
      images[i] = img
  return images, labels


# ---- guard bands and the comparison --------------------------------------------------------------------------------------
def guarded(shape, dtype, device):
  """(view, check, raw): a contiguous ``dtype`` tensor of ``shape`` inside one uint8 buffer filled with SENTINEL, GUARD_BYTES of
  guard on each side (the view is 256-byte aligned on the device).  ``check(name)`` asserts both bands still hold the
  sentinel.  The payload starts out sentinel-filled too, so an element a call must not write can be checked the same way."""
  n = 1
  for s in shape:
    n *= int(s)
  nbytes = n * torch.empty((), dtype=dtype).element_size()
  raw = torch.full((GUARD_BYTES + nbytes + GUARD_BYTES,), SENTINEL, dtype=torch.uint8, device=device)
  view = raw[GUARD_BYTES:GUARD_BYTES + nbytes].view(dtype).view(shape)

  def check(name):
    for side, part in (('in front of', raw[:GUARD_BYTES]), ('behind', raw[GUARD_BYTES + nbytes:])):
      hit = part != SENTINEL
      if bool(hit.any()):
        raise AssertionError('%s: wrote %s the buffer: %d guard bytes touched, first at %d' % (
            name, side, int(hit.sum()), int(hit.nonzero()[0])))

  return view, check, raw


def tensor_bits(t):
  """A bf16 / fp32 / int32 tensor's bit patterns as a NumPy array (uint16 / uint32 / int32)."""
  t = t.detach().contiguous().cpu()
  if t.dtype == torch.bfloat16:
    return t.view(torch.int16).numpy().view(np.uint16)
  if t.dtype == torch.float32:
    return t.view(torch.int32).numpy().view(np.uint32)
  return t.numpy()


def sentinel_of(np_dtype):
  return np.frombuffer(bytes([SENTINEL] * np.dtype(np_dtype).itemsize), dtype=np_dtype)[0]


def assert_same(name, got, want, batch_size):
  """The comparison of every test: ``got`` = the three output tensors (images, labels, indices) of ``batch_size`` slots,
  ``want`` = batch(...)'s result.  The first ``valid`` slots must equal the reference bit for bit; the others must still hold
  the sentinel they were allocated with."""
  w_bits, w_labels, w_idx, valid = want
  for what, t, w in (('images', got[0], w_bits), ('labels', got[1], w_labels), ('indices', got[2], w_idx)):
    g = tensor_bits(t).reshape((batch_size,) + w.shape[1:])
    assert g.dtype == w.dtype, (name, what, g.dtype, w.dtype)
    bad = g[:valid] != w
    if bad.any():
      first = np.argwhere(bad)[0].tolist()
      raise AssertionError('%s: %s: %d / %d elements differ in bits, first at %s: got %#x want %#x' % (
          name, what, int(bad.sum()), bad.size, first, int(g[:valid][tuple(first)]), int(w[tuple(first)])))
    assert (g[valid:] == sentinel_of(g.dtype)).all(), '%s: %s: a slot past the %d valid images was written' % (name, what, valid)
