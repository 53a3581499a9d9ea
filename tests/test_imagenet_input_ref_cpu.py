"""The NumPy specification of the ImageNet input pipeline (tests/imagenet_input_ref.py) on the CPU: hand-computed cases, the
conditions the case set must meet before a kernel is compared against it (asserted, not measured), the mutant pipelines the case set rejects, and the host
side of rigl_amd.data: store packing, save / load, the table refusals, the folder importer."""
import os

import numpy as np
import pytest

torch = pytest.importorskip('torch')

from tests import imagenet_input_ref as I  # noqa: E402

F = np.float32
Q0 = np.zeros(24, np.uint32)


def _fp32(bits):
  return bits.view(F)


# ---- hand-computed ---------------------------------------------------------------------------------------------------------
def test_one_pixel_image_fills_the_output_with_its_normalised_value():
  img = np.array([[[10, 20, 30]]], np.uint8)
  for train in (False, True):
    got = _fp32(I.image(img, Q0, 4, train, I.FP32))
    want = (np.array([10, 20, 30], F) - I.MEAN) / I.STD
    assert got.shape == (4, 4, 3) and (got == want).all()        # every tap is the pixel; the weights sum to exactly 1 at t = 0


def test_two_by_two_at_size_two_is_the_normalised_input():
  img = np.array([[[0, 1, 2], [3, 4, 5]], [[250, 251, 252], [253, 254, 255]]], np.uint8)
  assert I.centre_box(2, 2, 2) == (1, 1, 1, 1)                   # eval would crop (int)(f32(2/34) * 2) -> clamped to one pixel
  got = _fp32(I.resize(img, (0, 0, 2, 2), 2)[0])                 # the whole image as the box: scale 1, t = 0, weights 0 1 0 0
  assert (got == img.astype(F)).all()
  assert (I.normalise(got) == (img.astype(F) - I.MEAN) / I.STD).all()


def test_weights_sum_to_one_and_a_constant_image_stays_constant():
  for n_in, S in ((5, 8), (200, 32), (17, 224), (500, 224)):
    _, wt = I.taps(n_in, S)
    total = ((wt[:, 0] + wt[:, 1]) + wt[:, 2]) + wt[:, 3]
    # worst case, not a measurement: each weight takes 6 roundings of intermediates below 8 (half an ulp there = 2 eps), each
    # amplified by at most two later multiplications by x < 2 (x 4): 48 eps a weight, 192 for four, + 3 roundings of the sum
    assert np.abs(total - F(1)).max() <= 195 * np.finfo(F).eps
    assert (I.resize(np.full((n_in, n_in, 3), 128, np.uint8), (0, 0, n_in, n_in), S)[0][:, 0, 0] == F(128) * (
        ((wt[:, 0] + wt[:, 1]) + wt[:, 2]) + wt[:, 3]) * ((wt[0, 0] + wt[0, 1]) + wt[0, 2] + wt[0, 3])).all()
  img = np.full((10, 10, 3), 128, np.uint8)
  got = I.resize(img, (0, 0, 10, 10), 20)[0]                     # scale 0.5 exactly: t in {0, 0.5}, weights dyadic
  assert (got == F(128)).all()


def test_cubic_is_the_keys_kernel_at_its_knots():
  assert I.cubic(F(0)) == 1 and I.cubic(F(1)) == 0 and I.cubic(F(2)) == 0 and I.cubic(F(2.5)) == 0
  assert I.cubic(F(0.5)) == F(0.59375) and I.cubic(F(1.5)) == F(-0.09375)


def test_centre_crop_is_seven_eighths_at_224():
  assert F(224.0 / 256.0) == F(0.875)
  assert I.centre_box(375, 500, 224) == ((375 - 328 + 1) // 2, (500 - 328 + 1) // 2, 328, 328)
  assert I.centre_box(1, 1, 224) == (0, 0, 1, 1) and I.centre_box(3, 200, 224) == (1, 99, 2, 2)


def test_draws_do_not_depend_on_the_accepted_attempt():
  q = I.words(I.B_CASE, I.CASE_SEED, 0)
  assert q.shape == (8, 24)
  from tests import input_ref as R
  from oracle import tf_random as TR
  s0, s1 = TR.tf_seed_pair(0, I.CASE_SEED, 0)
  assert (q.reshape(-1) == TR.stateless_u32(192, s0, s1)).all()
  c = I.crop(64, 48, q[0], 32)
  if 0 <= c['attempt'] <= 9 and not c['whole']:
    assert c['box'][0] == int(q[0][20]) % (64 - c['box'][2] + 1) and c['box'][1] == int(q[0][21]) % (48 - c['box'][3] + 1)
  assert R._i32(-1) == -1


# ---- the case set ------------------------------------------------------------------------------------------------------------
def test_case_store_layout():
  store, offsets, dims, labels, arrays = I.case_store()
  assert len(arrays) == I.N_CASE == 67 and store.dtype == np.uint8
  sizes = set(map(tuple, dims.tolist()))
  assert set(I.PLANTED) <= sizes
  assert (offsets % 4 != 0).sum() > 10                           # unaligned images
  for j in (0, 5, 40, 66):
    assert (I.get_image(store, offsets, dims, j) == arrays[j]).all()


def test_case_set_meets_every_condition():
  p = I.properties(32)                                           # the crop sampler does not depend on S; the clamps and scales do
  assert all(v >= 3 for v in p.values()), p
  steps = (0, 7, 8, 15, 16)
  big, small = I.properties(224, steps), I.properties(8, steps)
  assert big['up'] >= 3 and big['bottom'] >= 3 and big['right'] >= 3 and small['down4'] >= 3, (big, small)


def test_checkerboard_overshoots_both_ways():
  v = I.resize(I.content('checker', 17, 23, None), (0, 0, 17, 23), 32)[0]
  assert v.min() < 0 and v.max() > 255


@pytest.mark.parametrize('mut', I.MUTANTS)
def test_case_set_rejects_the_mutant(mut):
  assert len(I.MUTANTS) >= 10
  differ = 0
  for step in range(I.STEPS_CASE):
    for train in (True, False):
      if not train and step >= 9:
        continue
      good = I.case_batch(step, I.BF16, 32, train)
      bad = I.case_batch(step, I.BF16, 32, train, mut=mut)
      differ += int((good[0] != bad[0]).sum())
  assert differ > 0, 'the case set cannot tell the %s pipeline from the specification' % mut


def test_rint_is_half_to_even_on_a_crafted_draw():
  """A tie in rintf needs hh * ar = k + 0.5 exactly, which no sampled draw of the case set produces (the twelfth mutant of the
  list, rintf as half-away, is therefore pinned here on chosen words and not by the case set): ar = 1.25 and hh = 2."""
  rng = F(4.0 / 3.0) - F(0.75)
  guess = int((0.5 / float(rng)) * (1 << 23))
  u = next(v for v in range(guess - 8, guess + 8) if I.u32_to_float(np.uint32(v)) * rng + F(0.75) == F(1.25))
  q = np.zeros(24, np.uint32)
  q[0:20:2], q[1:20:2] = u, 1                                    # r = 1: hh = 1 + 1 % 2 = 2, so ww = rintf(2.5)
  a, b = I.crop(2, 3, q, 8), I.crop(2, 3, q, 8, mut='rint_away')
  assert np.rint(F(2.5)) == 2 and a['box'][2:] == (2, 2) and b['whole']


def test_bad_rows_in_the_reference():
  store, offsets, dims, labels, _ = I.case_store()
  cut = int(offsets[40])                                         # rows 40 .. 66 end past this
  for b in range(9):
    bits, lab, ind, valid = I.batch(store, offsets, dims, labels, 8, b, I.FP32, 8, train=False, store_bytes=cut)
    for i in range(valid):
      j = 8 * b + i
      if j >= 40:
        assert lab[i] == -1 and ind[i] == -1 - j and not bits[i].any()
      else:
        assert lab[i] == labels[j] and ind[i] == j


# ---- rigl_amd.data: the store ------------------------------------------------------------------------------------------------
def test_pack_save_load_round_trip(tmp_path):
  from rigl_amd import data
  store, offsets, dims, labels, arrays = I.case_store()
  packed = data.pack_image_store(arrays, labels)
  for got, want in zip(packed, (store, offsets, dims, labels)):
    assert got.dtype == want.dtype and np.array_equal(got, want)
  data.save_image_store(str(tmp_path / 's'), *packed)
  assert sorted(os.listdir(str(tmp_path / 's'))) == sorted(data.STORE_FILES)
  for mmap in (True, False):
    loaded = data.load_image_store(str(tmp_path / 's'), mmap=mmap)
    assert isinstance(loaded[0], np.memmap) == mmap
    for got, want in zip(loaded, packed):
      assert got.dtype == want.dtype and np.array_equal(got, want)
  with pytest.raises(FileNotFoundError):
    data.load_image_store(str(tmp_path / 'none'))
  with pytest.raises(ValueError):
    data.pack_image_store([np.zeros((2, 2), np.uint8)], [0])
  with pytest.raises(ValueError):
    data.pack_image_store(arrays[:2], [0])


def test_table_refusals_name_the_first_bad_row():
  from rigl_amd import data
  store, offsets, dims, labels, _ = I.case_store()
  n = len(store)
  data.check_image_table(n, offsets, dims)

  def refused(row, **kw):
    o, d = offsets.copy(), dims.copy()
    if 'off' in kw:
      o[row] = kw['off']
    if 'h' in kw:
      d[row, 0] = kw['h']
    if 'w' in kw:
      d[row, 1] = kw['w']
    with pytest.raises(ValueError, match='row %d ' % row):
      data.check_image_table(kw.get('n', n), o, d)
  refused(3, h=0)
  refused(3, w=0)
  refused(5, h=4097)
  refused(5, w=-1)
  refused(7, off=-1)
  refused(66, off=int(offsets[66]) + 1)
  refused(2, off=np.iinfo(np.int64).max)
  refused(40, n=int(offsets[41]) - 1)
  with pytest.raises(ValueError):
    data.check_image_table(n, offsets, dims[:5])


def test_image_store_from_folder_reads_pngs_back_exactly(tmp_path):
  from PIL import Image
  from rigl_amd import data
  rng = np.random.RandomState(3)
  imgs = {('a', 'x.png'): rng.randint(0, 256, (5, 9, 3)), ('a', 'y.png'): rng.randint(0, 256, (12, 7, 3)),
          ('b', 'z.png'): rng.randint(0, 256, (1, 1, 3))}
  for (cls, name), a in imgs.items():
    os.makedirs(str(tmp_path / cls), exist_ok=True)
    Image.fromarray(a.astype(np.uint8)).save(str(tmp_path / cls / name))
  store, offsets, dims, labels, classes = data.image_store_from_folder(str(tmp_path))
  assert classes == ['a', 'b'] and labels.tolist() == [0, 0, 1] and dims.tolist() == [[5, 9], [12, 7], [1, 1]]
  for j, a in enumerate(imgs.values()):
    assert (I.get_image(store, offsets, dims, j) == a).all()
  _, _, dims8, _, _ = data.image_store_from_folder(str(tmp_path), short_side=10)
  assert [min(d) for d in dims8.tolist()] == [10, 10, 10]
  with pytest.raises(FileNotFoundError):
    data.image_store_from_folder(str(tmp_path / 'a'))
