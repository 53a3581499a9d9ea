"""TEST INFRASTRUCTURE: the NumPy specification of the device ImageNet input pipeline over rigl_amd.data's image store (DESIGN.md
section 4; the batch kernel that has to match it bit for bit is not in the tree): the distorted-bounding-box crop sampler, the centre crop, the legacy bicubic resize
(no half-pixel centres, Keys A = -0.75, taps clamped to the crop box), flip, normalisation and cast, every fp32 operation one
np.float32 operation (NumPy rounds + - * / sqrt rint floor and the conversions correctly, and never fuses).  Sample order and
the stateless stream come from tests/input_ref.py and oracle/tf_random.py.  Parity with TensorFlow itself is unpinned (as
tests/golden/tf_shim.py).  Never imported by the product.

  words(batch, seed0, step)            q0..q23 of every image of the batch
  crop(h, w, q, S, train, mut)         the crop box, the flip and how it came about
  resize(img, box, S, mut)             float32 [S, S, 3] and the clamps / scales it met
  image(img, q, S, train, dtype, mut)  one output image's bit patterns
  batch(store, ..., step, dtype, ...)  the whole call: (bits, labels, indices, valid), as input_ref.batch
  case_store()                         the seeded store the tests share; properties(...) counts what its draws cover
  MUTANTS                              pipelines that differ from the specification in one point; the case set rejects each
"""
import functools

import numpy as np

from oracle import tf_random as TR
from tests import input_ref as R
from tests.input_ref import BF16, FP32, TORCH_DTYPES, assert_same, guarded  # noqa: F401  (re-exported: a kernel test compares with these)

F = np.float32
KA = F(-0.75)
MEAN = np.array([0.485 * 255, 0.456 * 255, 0.406 * 255], dtype=np.float64).astype(F)
STD = np.array([0.229 * 255, 0.224 * 255, 0.225 * 255], dtype=np.float64).astype(F)
MAX_SIDE = 4096

MUTANTS = ('half_pixel', 'a_half', 'clamp_image', 'vertical_first', 'fma', 'reciprocal', 'bf16_trunc', 'flip_before_crop',
           'attempt_xy', 'no_cover', 'centre_floor')     # 'rint_away' exists too; only a crafted draw can show it


# ---- draws -----------------------------------------------------------------------------------------------------------------
def words(batch_size, seed0, step):
  """uint32 [batch, 24]: image i owns Philox blocks 6i .. 6i+5 of stateless_u32 under the seed pair [seed0, step]."""
  s0, s1 = TR.tf_seed_pair(0, int(seed0), R._i32(step))
  return TR.stateless_u32(24 * int(batch_size), s0, s1).reshape(-1, 24)


def u32_to_float(x):
  return ((np.uint32(127) << np.uint32(23)) | (np.uint32(x) & np.uint32(0x7FFFFF))).view(F) - F(1.0)


def _rint(x, mut):
  if mut == 'rint_away':                                   # mutant: halves away from zero
    x = np.float64(x)
    return F(np.sign(x) * np.floor(np.abs(x) + 0.5))
  return np.rint(F(x))


# ---- crop ------------------------------------------------------------------------------------------------------------------
def centre_box(h, w, S, mut=None):
  ratio = F(np.float64(S) / (np.float64(S) + 32.0))
  size = max(1, int(ratio * F(min(h, w))))
  if mut == 'centre_floor':                                # mutant: offset (h - size) / 2
    return (h - size) // 2, (w - size) // 2, size, size
  return (h - size + 1) // 2, (w - size + 1) // 2, size, size


def crop(h, w, q, S, train=True, mut=None):
  """dict(box=(y0, x0, hh, ww), flip, attempt): attempt = the accepted attempt 0..9, 10 when all were rejected, -1 in eval;
  whole = the accepted box was the whole image (the centre crop stands in both fallbacks)."""
  h, w = int(h), int(w)
  out = dict(box=centre_box(h, w, S, mut), flip=False, attempt=-1, whole=False)
  if not train:
    return out
  out['flip'] = bool(u32_to_float(q[22]) < F(0.5))
  out['attempt'] = 10
  A = F(h * w)
  min_area, max_area, cover = F(0.08) * A, A, F(0.1) * A
  rng = F(4.0 / 3.0) - F(0.75)
  for a in range(10):
    u, r = q[2 * a], int(q[2 * a + 1])
    ar = u32_to_float(u) * rng + F(0.75)
    hh = int(_rint(np.sqrt(min_area / ar), mut))
    mh = int(_rint(np.sqrt(max_area / ar), mut))
    if _rint(F(mh) * ar, mut) > F(w):
      mh = int((F(w) + F(0.5)) / ar)
      if _rint(F(mh) * ar, mut) > F(w):
        mh -= 1
    mh = min(mh, h)
    hh = min(hh, mh)
    if hh < mh:
      hh += r % (mh - hh + 1)
    ww = int(_rint(F(hh) * ar, mut))
    area = F(ww * hh)
    if area < min_area:
      hh += 1
      ww = int(_rint(F(hh) * ar, mut))
      area = F(ww * hh)
    if area > max_area:
      hh -= 1
      ww = int(_rint(F(hh) * ar, mut))
      area = F(ww * hh)
    if area < min_area or area > max_area or ww > w or hh > h or ww <= 0 or hh <= 0:
      continue
    if mut != 'no_cover' and area < cover:                 # mutant: min_object_covered dropped
      continue
    out['attempt'] = a
    if ww == w and hh == h:
      out['whole'] = True
      return out
    qy, qx = (int(q[2 * a]), int(q[2 * a + 1])) if mut == 'attempt_xy' else (int(q[20]), int(q[21]))
    out['box'] = (qy % (h - hh + 1), qx % (w - ww + 1), hh, ww)
    return out
  return out


# ---- resize ----------------------------------------------------------------------------------------------------------------
def cubic(x, A=KA):
  x = np.asarray(x, dtype=F)
  near = (((A + F(2)) * x - (A + F(3))) * x) * x + F(1)
  far = ((A * x - F(5) * A) * x + F(8) * A) * x - F(4) * A
  return np.where(x <= F(1), near, np.where(x < F(2), far, F(0))).astype(F)


def taps(n_in, S, mut=None):
  """(index [S, 4] into the box, unclamped; weights [S, 4] float32) of one axis of the resize."""
  scale = F(n_in) / F(S)
  o = np.arange(S).astype(F)
  pos = (o + F(0.5)) * scale - F(0.5) if mut == 'half_pixel' else o * scale
  fl = np.floor(pos)
  t = pos - fl
  A = F(-0.5) if mut == 'a_half' else KA
  wt = np.stack([cubic(F(1) + t, A), cubic(t, A), cubic(F(1) - t, A), cubic(F(2) - t, A)], axis=1)
  return fl.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :], wt


def _acc(w, p, mut):
  """((w0 p0 + w1 p1) + w2 p2) + w3 p3 along the last axis (length 4)."""
  s = (w[..., 0] * p[..., 0] + w[..., 1] * p[..., 1]) + w[..., 2] * p[..., 2]
  if mut == 'fma':                                         # mutant: the last accumulation contracted to one rounding
    return (np.float64(w[..., 3]) * np.float64(p[..., 3]) + np.float64(s)).astype(F)
  return s + w[..., 3] * p[..., 3]


def resize(img, box, S, mut=None):
  """(float32 [S, S, 3], info): the box of ``img`` (uint8 [h, w, 3]) resized; info = which sides clamped a tap and the scales."""
  y0, x0, hh, ww = box
  h, w = img.shape[:2]
  ri, rw = taps(hh, S, mut)
  ci, cw = taps(ww, S, mut)
  info = dict(top=bool((ri < 0).any()), bottom=bool((ri > hh - 1).any()), left=bool((ci < 0).any()),
              right=bool((ci > ww - 1).any()), scale=max(hh, ww) / float(S), up=hh < S and ww < S)
  if mut == 'clamp_image':                                 # mutant: taps clamped to the image, not the crop box
    rows, cols = np.clip(ri + y0, 0, h - 1), np.clip(ci + x0, 0, w - 1)
  else:
    rows, cols = np.clip(ri, 0, hh - 1) + y0, np.clip(ci, 0, ww - 1) + x0
  if mut == 'vertical_first':
    used, inv = np.unique(cols, return_inverse=True)
    p = img[:, used].astype(F)[rows]                       # [S, 4, ncols, 3]
    v = _acc(rw[:, None, None, :], np.moveaxis(p, 1, -1), None)        # [S, ncols, 3]
    g = v[:, inv.reshape(cols.shape)]                      # [S, S, 4, 3]
    return _acc(cw[None, :, None, :], np.moveaxis(g, 2, -1), None), info
  used, inv = np.unique(rows, return_inverse=True)
  p = img[used][:, cols].astype(F)                         # [nrows, S, 4, 3]
  hres = _acc(cw[None, :, None, :], np.moveaxis(p, 2, -1), mut)        # [nrows, S, 3]
  g = hres[inv.reshape(rows.shape)]                        # [S, 4, S, 3]
  return _acc(rw[:, None, None, :], np.moveaxis(g, 1, -1), mut), info


def normalise(v, mut=None):
  if mut == 'reciprocal':                                  # mutant: multiply by 1 / std
    return ((v - MEAN) * (F(1) / STD)).astype(F)
  return ((v - MEAN) / STD).astype(F)


def image(img, q, S, train=True, dtype=BF16, mut=None, info=None):
  """One output image: bit patterns [S, S, 3] (uint16 for bf16, uint32 for fp32).  ``info``, a dict, receives the crop and
  resize facts properties() counts."""
  h, w = img.shape[:2]
  c = crop(h, w, q, S, train, mut)
  if mut == 'flip_before_crop' and c['flip']:              # mutant: the box is taken from the flipped image
    img = img[:, ::-1]
    v, ri = resize(img, c['box'], S, mut)
  else:
    v, ri = resize(img, c['box'], S, mut)
    if c['flip']:
      v = v[:, ::-1]
  if info is not None:
    info.update(c)
    info.update(ri)
  y = normalise(v, mut)
  if dtype == BF16:
    return R.bf16_bits(y, 'trunc' if mut == 'bf16_trunc' else 'rne')
  return np.ascontiguousarray(y, dtype=F).view(np.uint32).copy()


# ---- the whole call ---------------------------------------------------------------------------------------------------------
def row_ok(store_bytes, off, h, w):
  return 1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE and off >= 0 and off + 3 * h * w <= store_bytes


def get_image(store, offsets, dims, j):
  h, w = int(dims[j, 0]), int(dims[j, 1])
  o = int(offsets[j])
  return np.asarray(store[o:o + 3 * h * w]).reshape(h, w, 3)


def indices(n, batch_size, step, train=True, seed0=0, shard=0, n_shards=1):
  if train:
    return R.train_indices(n, batch_size, seed0, step, shard, n_shards)
  return R.eval_indices(n, batch_size, step, shard, n_shards)[0]


def batch(store, offsets, dims, labels, batch_size, step, dtype, S, train=True, seed0=0, shard=0, n_shards=1, store_bytes=None,
          mut=None, infos=None):
  """(bits [valid, S, S, 3], labels [valid] int32, indices [valid] int32, valid).  A row that is bad against ``store_bytes``
  gives zeros, label -1 and index -1 - index."""
  nbytes = len(store) if store_bytes is None else int(store_bytes)
  idx = indices(len(offsets), batch_size, step, train, seed0, shard, n_shards)
  q = words(batch_size, seed0, step)
  out = np.zeros((len(idx), S, S, 3), dtype=np.uint16 if dtype == BF16 else np.uint32)
  lab, ind = np.empty(len(idx), np.int32), np.empty(len(idx), np.int32)
  for i, j in enumerate(idx):
    if not row_ok(nbytes, int(offsets[j]), int(dims[j, 0]), int(dims[j, 1])):
      lab[i], ind[i] = -1, -1 - j
      continue
    info = {} if infos is not None else None
    out[i] = image(get_image(store, offsets, dims, j), q[i], S, train, dtype, mut, info)
    lab[i], ind[i] = labels[j], j
    if infos is not None:
      infos.append(info)
  return out, lab, ind, len(idx)


# ---- the case store ----------------------------------------------------------------------------------------------------------
PLANTED = [(1, 1), (1, 7), (7, 1), (2, 2), (4, 4), (5, 4), (3, 200), (200, 3), (17, 23), (64, 48), (375, 500), (500, 375)]
KINDS = ('random', 'zeros', 'all255', 'checker', 'ramp')
N_CASE, B_CASE, STEPS_CASE = 67, 8, 18                     # 8 steps per epoch, 3 positions skipped; eval: 9 batches, the last of 3
CASE_SEED = 7


def content(kind, h, w, rng):
  if kind == 'zeros':
    return np.zeros((h, w, 3), np.uint8)
  if kind == 'all255':
    return np.full((h, w, 3), 255, np.uint8)
  if kind == 'checker':                                    # bicubic overshoot below 0 and above 255
    yy, xx = np.mgrid[0:h, 0:w]
    return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
  if kind == 'ramp':
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(xx * 7 + yy) % 256, (yy * 5 + 2 * xx) % 256, (xx + yy) * 255 // max(1, h + w - 2)], axis=2).astype(np.uint8)
  return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def case_store():
  """(store, offsets, dims, labels, arrays): 67 images -- every planted size three times with rotating contents (the large
  two twice), then random sizes from 6 to 160 -- packed back to back, so most images start at an odd address."""
  rng = np.random.RandomState(2024)
  sizes = []
  for rep in range(3):
    sizes += [(s, KINDS[(k + 2 * rep) % len(KINDS)]) for k, s in enumerate(PLANTED) if rep < 2 or max(s) < 300]
  while len(sizes) < N_CASE:
    sizes.append(((int(rng.randint(6, 161)), int(rng.randint(6, 161))), KINDS[len(sizes) % len(KINDS)]))
  arrays = [content(kind, h, w, rng) for (h, w), kind in sizes]
  labels = rng.randint(0, 1000, len(arrays)).astype(np.int32)
  dims = np.array([a.shape[:2] for a in arrays], dtype=np.int32)
  nbytes = 3 * dims[:, 0].astype(np.int64) * dims[:, 1]
  offsets = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
  store = np.concatenate([a.reshape(-1) for a in arrays])
  return store, offsets, dims, labels, arrays


@functools.lru_cache(maxsize=None)
def case_batch(step, dtype, S, train=True, seed0=CASE_SEED, shard=0, n_shards=1, batch_size=B_CASE, mut=None):
  """batch() over the case store, computed once per argument set and shared by the tests (treat the arrays as read-only)."""
  store, offsets, dims, labels, _ = case_store()
  infos = []
  out = batch(store, offsets, dims, labels, batch_size, step, dtype, S, train, seed0, shard, n_shards, mut=mut, infos=infos)
  return out + (infos,)


def properties(S, steps=range(STEPS_CASE)):
  """How many images of the train case (the case store, B_CASE, CASE_SEED, ``steps``) meet each condition the tests demand."""
  count = dict(first=0, later=0, none=0, whole=0, flipped=0, unflipped=0, top=0, bottom=0, left=0, right=0, up=0, down4=0)
  for s in steps:
    for f in case_batch(s, BF16, S)[4]:
      count['first'] += f['attempt'] == 0
      count['later'] += 1 <= f['attempt'] <= 9
      count['none'] += f['attempt'] == 10
      count['whole'] += f['whole']
      count['flipped'] += f['flip']
      count['unflipped'] += not f['flip']
      for side in ('top', 'bottom', 'left', 'right'):
        count[side] += f[side]
      count['up'] += f['up']
      count['down4'] += f['scale'] > 4
  return count
