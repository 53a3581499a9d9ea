"""tests/input_ref.py (the NumPy reference of rigl_cifar_batch) checked without a GPU: the standardization against an fp64
statement of tf.image.per_image_standardization, the index map against np.pad, the sample order's bijectivity and mixing, a
set of mutants that the GPU tests' comparison must reject, and rigl_amd.data.load_cifar10_python."""
import pickle

import numpy as np
import pytest

torch = pytest.importorskip('torch')

from tests import input_ref as R  # noqa: E402

N, B, STEPS = 37, 8, 10            # the GPU test's train case


# ---- standardization -----------------------------------------------------------------------------------------------------
def _tf64(img):
  """(x - mean) / max(stddev, 1 / sqrt(n)) in fp64."""
  x = img.astype(np.float64)
  mean = x.mean()
  std = np.sqrt(((x - mean) ** 2).mean())
  return (x - mean) / max(std, 1.0 / np.sqrt(x.size))


@pytest.mark.parametrize('name', sorted(R.edge_images()))
def test_standardization_against_fp64(name):
  """fp32: one int -> fp32 conversion, sqrtf, one division and one multiply, each <= 2^-24 relative: under 2^-21 in total, the
  bound 2^-20 leaves a factor of two.  bf16 adds one half-ulp of its 8-bit significand: 2^(e - 8) for a value in [2^e, 2^(e+1))."""
  img = R.edge_images()[name]
  want = _tf64(img)
  y32 = R.standardize(img)
  assert y32.dtype == np.float32
  ybf = (R.bf16_bits(y32).astype(np.uint32) << np.uint32(16)).view(np.float32)
  half_ulp = np.where(want != 0, np.ldexp(1.0, np.frexp(want)[1] - 9), 0.0)        # frexp: |want| in [2^(e-1), 2^e)
  for what, got, extra in (('fp32', y32, 0.0), ('bf16', ybf, half_ulp)):
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / np.maximum(np.abs(want), 1e-300))[want != 0].max()) if (want != 0).any() else 0.0
    print('%s %s: largest relative difference 2^%.1f' % (name, what, np.log2(max(worst, 1e-30))))
    assert (err <= 2.0 ** -20 * np.abs(want) + extra).all(), (name, what, worst)
  if name in ('zeros', 'all255'):
    assert (y32.view(np.uint32) == 0).all() and (R.bf16_bits(y32) == 0).all()       # +0, not -0, not NaN


def test_single_pixel_images_sit_on_the_stddev_floor():
  for name in ('one_in_zeros', 'one254_in_255'):
    x = R.edge_images()[name].astype(np.int64)
    d = R.N_PIX * int((x * x).sum()) - int(x.sum()) ** 2
    assert d == R.N_PIX - 1                                  # sqrt(3071) < sqrt(3072): the floor applies
    assert not np.array_equal(R.standardize(x.astype(np.uint8)), R.standardize(x.astype(np.uint8), floor=False))


def test_bf16_rounding_is_nearest_even():
  v = np.array([0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0xBF818000], dtype=np.uint32).view(np.float32)
  assert R.bf16_bits(v).tolist() == [0x3F80, 0x3F82, 0x3F81, 0x3F80, 0xBF80, 0xBF82]
  assert R.bf16_bits(v, mode='trunc').tolist() == [0x3F80, 0x3F81, 0x3F80, 0x3F80, 0xBF80, 0xBF81]


# ---- index map -----------------------------------------------------------------------------------------------------------
def test_index_map_equals_symmetric_pad_crop_flip():
  img = np.arange(R.N_PIX, dtype=np.int64).reshape(R.SIDE, R.SIDE, R.CH)               # distinct values
  padded = np.pad(img, ((4, 4), (4, 4), (0, 0)), mode='symmetric')
  for oy in range(9):
    for ox in range(9):
      for flip in (False, True):
        want = padded[oy:oy + 32, ox:ox + 32]
        if flip:
          want = want[:, ::-1]
        assert np.array_equal(R.augment(img, oy, ox, flip), want), (oy, ox, flip)
  assert np.array_equal(R.augment(img, 4, 4, False), img)                               # eval mode's map


def test_host_restatements_agree_with_the_index_map():
  from rigl.cifar_resnet import data_helper as DH
  img = np.arange(R.N_PIX, dtype=np.float32).reshape(R.SIDE, R.SIDE, R.CH)
  assert DH.IMG_SIZE == 32 and DH.pad_input(img).shape == (40, 40, 3)
  assert np.array_equal(DH.pad_input(img)[:, :, 0][0, :6], img[3, [3, 2, 1, 0, 0, 1], 0])
  for oy, ox, flip in ((0, 8, True), (8, 0, False), (4, 4, False), (3, 5, True)):
    assert np.array_equal(DH.preprocess_train(img, 32, 32, offset=(oy, ox), flip=flip), R.augment(img, oy, ox, flip))
  assert DH.preprocess_train(img, 32, 32, rng=np.random.RandomState(0)).shape == (32, 32, 3)


# ---- sample order --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 2, 3, 5, 37, 128, 1000, 50000])
def test_order_is_a_bijection(n):
  for epoch in (0, 1, 7):
    perm = R.order(n, 1234, epoch, np.arange(n))
    assert np.array_equal(np.sort(perm), np.arange(n)), (n, epoch)


def test_order_mixes_at_cifar_size():
  n = 50000
  p = np.arange(n)
  perm = R.order(n, 1234, 0, p)
  corr = float(np.corrcoef(p, perm)[0, 1])
  jump = float(np.abs(np.diff(perm)).mean() / n)
  print('corr %.4f, mean |pi(p+1) - pi(p)| / N %.4f' % (corr, jump))
  assert abs(corr) <= 0.05
  assert 0.31 <= jump <= 0.36
  assert not (perm == R.order(n, 1234, 1, p)).all()


def test_one_epoch_visits_distinct_images_and_the_next_is_reshuffled():
  assert R.steps_per_epoch(N, B) == 4
  epoch0 = np.concatenate([R.train_indices(N, B, 7, s) for s in range(4)])
  assert len(set(epoch0.tolist())) == 32 and epoch0.min() >= 0 and epoch0.max() < N
  assert np.array_equal(epoch0, R.order(N, 7, 0, np.arange(32)))
  epoch1 = np.concatenate([R.train_indices(N, B, 7, s) for s in range(4, 8)])
  assert len(set(epoch1.tolist())) == 32 and not np.array_equal(epoch0, epoch1)


def test_shards_partition_the_single_shard_batch():
  for step in (0, 3, 4, 9):
    whole = R.train_indices(N, 8, 7, step)
    a, b = R.train_indices(N, 4, 7, step, 0, 2), R.train_indices(N, 4, 7, step, 1, 2)
    assert not set(a.tolist()) & set(b.tolist())
    assert np.array_equal(np.concatenate([a, b]), whole)


def test_eval_indices():
  assert [R.eval_indices(N, B, b)[1] for b in range(6)] == [8, 8, 8, 8, 5, 0]
  assert R.eval_indices(N, B, 4)[0].tolist() == [32, 33, 34, 35, 36]
  assert R.eval_indices(N, B, 1, shard=1, n_shards=2)[0].tolist() == list(range(24, 32))
  assert R.eval_indices(N, B, 2, shard=0, n_shards=2)[0].tolist() == [32, 33, 34, 35, 36]


def test_train_seed_covers_the_corners():
  """The GPU test's seed: its 80 draws hold every corner offset with and without flip, and the centre unflipped."""
  assert R.corner_coverage_missing(B, R.TRAIN_SEED, range(STEPS)) == []


# ---- mutants -------------------------------------------------------------------------------------------------------------
def _emulate(images, labels, step, dtype, kind=None):
  """What a kernel with one mistake would leave in guarded output buffers (CPU tensors) for the train batch at ``step``."""
  idx = R.train_indices(N, B, R.TRAIN_SEED, step)
  oy, ox, flip = R.draws(B, R.TRAIN_SEED, step)
  out, check_out, _ = R.guarded((B, 32, 32, 3), R.TORCH_DTYPES[dtype], 'cpu')
  lab, check_lab, _ = R.guarded((B,), torch.int32, 'cpu')
  ind, check_ind, raw_ind = R.guarded((B,), torch.int32, 'cpu')
  bits = np.empty((B, 32, 32, 3), dtype=np.uint16 if dtype == R.BF16 else np.uint32)
  for i, j in enumerate(idx):
    a, b, f = int(oy[i]), int(ox[i]), bool(flip[i])
    if kind == 'reflect':
      y = np.pad(R.standardize(images[j]), ((4, 4), (4, 4), (0, 0)), mode='reflect')[a:a + 32, b:b + 32]
      y = y[:, ::-1] if f else y
    elif kind == 'no_floor':
      y = R.augment(R.standardize(images[j], floor=False), a, b, f)
    elif kind == 'crop_statistics':
      y = R.standardize(R.augment(images[j], a, b, f))
    elif kind == 'swapped_offsets':
      y = R.augment(R.standardize(images[j]), b, a, f)
    elif kind == 'flip_before_crop':
      c = np.arange(32)
      cols = R.source(2 * R.PAD + R.SIDE - 1 - (c + b)) if f else R.source(c + b)
      y = R.standardize(images[j])[R.source(c + a)][:, cols]
    else:
      y = R.augment(R.standardize(images[j]), a, b, f)
    bits[i] = R.bf16_bits(y, mode='trunc') if (kind == 'truncate' and dtype == R.BF16) else R.out_bits(y, dtype)
  view = torch.int16 if dtype == R.BF16 else torch.int32
  out.view(view).copy_(torch.from_numpy(bits.view(np.int16 if dtype == R.BF16 else np.int32)))
  lab.copy_(torch.from_numpy(labels[idx]))
  ind.copy_(torch.from_numpy(idx.astype(np.int32)))
  if kind == 'store_past_the_end':
    raw_ind[R.GUARD_BYTES + 4 * B] = 0                       # the first byte of out_index[batch]
  return (out, lab, ind), (check_out, check_lab, check_ind)


def _accepted(images, labels, dtype, kind):
  """True if the GPU test's comparison passes on every step 0..9 for this emulation."""
  for step in range(STEPS):
    got, checks = _emulate(images, labels, step, dtype, kind)
    try:
      for c in checks:
        c(kind)
      R.assert_same('step %d' % step, got, R.batch(images, labels, B, step, dtype, seed0=R.TRAIN_SEED), B)
    except AssertionError:
      return False
  return True


@pytest.fixture(scope='module')
def small():
  return R.dataset(N)


@pytest.mark.parametrize('dtype', [R.BF16, R.FP32])
def test_faithful_emulation_is_accepted(small, dtype):
  assert _accepted(small[0], small[1], dtype, None)


@pytest.mark.parametrize('kind', ['reflect', 'no_floor', 'crop_statistics', 'swapped_offsets', 'flip_before_crop', 'truncate',
                                  'store_past_the_end'])
def test_mutant_is_rejected(small, kind):
  assert not _accepted(small[0], small[1], R.BF16, kind)
  if kind != 'truncate':
    assert not _accepted(small[0], small[1], R.FP32, kind)


def test_eval_partial_batch_must_leave_the_tail_untouched(small):
  images, labels = small
  want = R.batch(images, labels, B, 4, R.BF16, train=False)
  assert want[3] == 5
  out, _, _ = R.guarded((B, 32, 32, 3), torch.bfloat16, 'cpu')
  lab, _, _ = R.guarded((B,), torch.int32, 'cpu')
  ind, _, _ = R.guarded((B,), torch.int32, 'cpu')
  out.view(torch.int16)[:5].copy_(torch.from_numpy(want[0].view(np.int16)))
  lab[:5].copy_(torch.from_numpy(want[1]))
  ind[:5].copy_(torch.from_numpy(want[2]))
  R.assert_same('eval', (out, lab, ind), want, B)
  lab[6] = 0                                                 # a kernel that wrote a slot past the dataset's end
  with pytest.raises(AssertionError):
    R.assert_same('eval', (out, lab, ind), want, B)


# ---- the CIFAR-10 python pickles -----------------------------------------------------------------------------------------
def test_load_cifar10_python(tmp_path):
  from rigl_amd import data
  rng = np.random.RandomState(3)
  hwc = rng.randint(0, 256, (7, 32, 32, 3)).astype(np.uint8)
  lab = rng.randint(0, 10, 7)
  d = tmp_path / 'cifar-10-batches-py'
  d.mkdir()
  for name, sl in (('data_batch_2', slice(4, 7)), ('data_batch_1', slice(0, 4))):
    planar = hwc[sl].transpose(0, 3, 1, 2).reshape(-1, 3072)           # rows of 1024 R, 1024 G, 1024 B
    with open(str(d / name), 'wb') as f:
      pickle.dump({b'data': planar, b'labels': [int(v) for v in lab[sl]], b'batch_label': b'x'}, f)
  images, labels = data.load_cifar10_python(str(d))
  assert images.dtype == np.uint8 and images.flags['C_CONTIGUOUS'] and labels.dtype == np.int32
  assert np.array_equal(images, hwc) and np.array_equal(labels, lab)
  with pytest.raises(FileNotFoundError, match='does not exist'):
    data.load_cifar10_python(str(tmp_path / 'absent'))
  with pytest.raises(FileNotFoundError, match='no test_batch'):
    data.load_cifar10_python(str(d), 'eval')
