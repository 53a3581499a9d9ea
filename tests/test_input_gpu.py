"""rigl_cifar_batch / rigl_cifar_advance on the GPU: zero differing bits against tests/input_ref.py -- images, labels and dataset
indices, train and eval, bf16 and fp32 -- inside sentinel bands, with the dataset unchanged; the device counter; and every
argument error, reported before anything is launched."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')

from tests import input_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N, B, STEPS = 37, 8, 10


@functools.lru_cache(maxsize=None)
def _data(n):
  """(images, labels) NumPy, their device copies, and pristine device clones to compare against afterwards."""
  images, labels = R.dataset(n)
  d_img, d_lab = torch.from_numpy(images).to(DEV), torch.from_numpy(labels).to(DEV)
  return images, labels, d_img, d_lab, d_img.clone(), d_lab.clone()


def _outputs(batch, dtype):
  out, c0, _ = R.guarded((batch, 32, 32, 3), R.TORCH_DTYPES[dtype], DEV)
  lab, c1, _ = R.guarded((batch,), torch.int32, DEV)
  ind, c2, _ = R.guarded((batch,), torch.int32, DEV)

  def check(name):
    for c in (c0, c1, c2):
      c(name)
  return (out, lab, ind), check


def _call(n, batch, step, dtype, **kw):
  """One rigl_cifar_batch into fresh guarded outputs; bands and dataset checked.  Returns the three output tensors."""
  from rigl_amd import ops
  _, _, d_img, d_lab, img0, lab0 = _data(n)
  got, check = _outputs(batch, dtype)
  step_t = torch.full((1,), step, dtype=torch.int32, device=DEV)
  ops.cifar_batch(d_img, d_lab, batch, step_t, got[0], got[1], out_index=got[2], **kw)
  torch.cuda.synchronize()
  check('step %d %r' % (step, kw))
  assert torch.equal(d_img, img0) and torch.equal(d_lab, lab0), 'the dataset was written'
  assert int(step_t) == step                                   # the batch kernel only reads the counter
  return got


# ---- train mode ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [R.BF16, R.FP32], ids=['bf16', 'fp32'])
def test_train_batches_are_bit_exact_across_epoch_boundaries(dtype):
  images, labels = _data(N)[:2]
  assert R.corner_coverage_missing(B, R.TRAIN_SEED, range(STEPS)) == []          # before anything is compared
  seen = set()
  for step in range(STEPS):                                     # 4 steps per epoch: boundaries after steps 3 and 7
    want = R.batch(images, labels, B, step, dtype, seed0=R.TRAIN_SEED)
    R.assert_same('train step %d' % step, _call(N, B, step, dtype, seed0=R.TRAIN_SEED), want, B)
    seen |= set(want[2].tolist())
  assert set(R.planted_indices(N)) <= seen                      # every planted edge image was drawn


@pytest.mark.parametrize('step', [-1, (1 << 31) - 1])
def test_train_step_is_read_as_its_bit_pattern(step):
  images, labels = _data(N)[:2]
  want = R.batch(images, labels, B, step, R.BF16, seed0=-1201226755)
  R.assert_same('train step %d' % step, _call(N, B, step, R.BF16, seed0=-1201226755), want, B)


def test_train_shards_are_bit_exact_and_disjoint():
  images, labels = _data(N)[:2]
  idx = []
  for shard in (0, 1):
    want = R.batch(images, labels, 4, 5, R.BF16, seed0=R.TRAIN_SEED, shard=shard, n_shards=2)
    got = _call(N, 4, 5, R.BF16, seed0=R.TRAIN_SEED, shard=shard, n_shards=2)
    R.assert_same('shard %d' % shard, got, want, 4)
    idx.append(got[2].cpu().numpy())
  assert np.array_equal(np.concatenate(idx), R.train_indices(N, 8, R.TRAIN_SEED, 5))


@pytest.mark.parametrize('batch', [1, 3, 5])                     # fewer images than a workgroup's four waves, and one more
def test_train_batches_that_do_not_fill_a_workgroup(batch):
  images, labels = _data(N)[:2]
  want = R.batch(images, labels, batch, 2, R.FP32, seed0=11)
  R.assert_same('batch %d' % batch, _call(N, batch, 2, R.FP32, seed0=11), want, batch)


def test_train_cifar_size_sixteen_bit_domain():
  n, batch = 50000, 128
  images, labels = _data(n)[:2]
  assert R.half_bits(n) == 8 and R.steps_per_epoch(n, batch) == 390
  for step in (0, 390):                                          # the first batch of epochs 0 and 1
    want = R.batch(images, labels, batch, step, R.BF16, seed0=1234)
    R.assert_same('N 50000 step %d' % step, _call(n, batch, step, R.BF16, seed0=1234), want, batch)


# ---- eval mode -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [R.BF16, R.FP32], ids=['bf16', 'fp32'])
def test_eval_batches_and_the_partial_tail(dtype):
  images, labels = _data(N)[:2]
  for b in range(5):
    want = R.batch(images, labels, B, b, dtype, train=False)
    assert want[3] == (8 if b < 4 else 5)
    assert want[2].tolist() == list(range(8 * b, min(8 * b + 8, N)))
    R.assert_same('eval batch %d' % b, _call(N, B, b, dtype, train=False), want, B)      # slots past 5 keep the sentinel
  assert R.batch(images, labels, B, 5, dtype, train=False)[3] == 0
  R.assert_same('eval batch 5', _call(N, B, 5, dtype, train=False), R.batch(images, labels, B, 5, dtype, train=False), B)


def test_eval_shards():
  images, labels = _data(N)[:2]
  for shard in (0, 1):
    for b in range(3):
      want = R.batch(images, labels, B, b, R.BF16, train=False, shard=shard, n_shards=2)
      R.assert_same('eval shard %d batch %d' % (shard, b), _call(N, B, b, R.BF16, train=False, shard=shard, n_shards=2), want, B)
  assert R.batch(images, labels, B, 2, R.BF16, train=False, shard=0, n_shards=2)[3] == 5
  assert R.batch(images, labels, B, 2, R.BF16, train=False, shard=1, n_shards=2)[3] == 0


# ---- the counter ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('step', [0, 5, -1, (1 << 31) - 1])
def test_advance_moves_the_counter_by_one(step):
  from rigl_amd import ops
  view, check, _ = R.guarded((1,), torch.int32, DEV)
  view.fill_(step)
  ops.cifar_advance(view)
  torch.cuda.synchronize()
  check('advance')
  assert int(view) == (step + 1 if step + 1 < (1 << 31) else -(1 << 31))


def test_device_cifar_counts_seeks_and_reports():
  from rigl_amd import data
  images, labels = _data(N)[:2]
  dc = data.DeviceCifar(images, labels, B, seed=R.TRAIN_SEED, device=DEV, with_indices=True)
  assert dc.steps_per_epoch == 4 and dc.position() == 0
  dc.seek(3)
  assert dc.position() == 3
  for s in (3, 4):                                               # two calls: steps s and s + 1, across the epoch boundary
    x, y = dc.next_batch()
    assert x is dc.images and y is dc.labels and y.dtype == torch.int64
    want = R.batch(images, labels, B, s, R.BF16, seed0=R.TRAIN_SEED)
    assert np.array_equal(R.tensor_bits(x), want[0])
    assert np.array_equal(y.cpu().numpy(), want[1]) and np.array_equal(dc.last_indices().cpu().numpy(), want[2])
    assert dc.position() == s + 1
  dc.seek(-1)
  assert dc.position() == -1
  ev = data.DeviceCifar(images, labels, B, train=False, device=DEV, dtype=torch.float32)
  assert ev.steps_per_epoch == 5 and [ev.valid_count(b) for b in range(6)] == [8, 8, 8, 8, 5, 0]
  ev.seek(4)
  x, y = ev.next_batch()
  want = R.batch(images, labels, B, 4, R.FP32, train=False)
  assert np.array_equal(R.tensor_bits(x)[:5], want[0]) and np.array_equal(y.cpu().numpy()[:5], want[1])
  with pytest.raises(ValueError):
    ev.last_indices()
  with pytest.raises(ValueError):
    data.DeviceCifar(images, labels, 64, device=DEV)            # train mode needs a whole batch


# ---- argument errors -----------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing():
  from rigl_amd import _lib
  lib = _lib.load()
  _, _, d_img, d_lab, img0, lab0 = _data(N)
  got, check = _outputs(B, R.BF16)
  step_t = torch.zeros(1, dtype=torch.int32, device=DEV)
  p = lambda t: C.c_void_p(t.data_ptr())
  good = dict(images=p(d_img), labels=p(d_lab), n=N, batch=B, mode=0, shard=0, n_shards=1, seed0=1, step=p(step_t), out=p(got[0]),
              dtype=0, out_labels=p(got[1]), out_index=p(got[2]))
  order = ['images', 'labels', 'n', 'batch', 'mode', 'shard', 'n_shards', 'seed0', 'step', 'out', 'dtype', 'out_labels', 'out_index']
  cases = [dict(images=None), dict(labels=None), dict(step=None), dict(out=None), dict(out_labels=None),
           dict(batch=0), dict(batch=-3), dict(n=0), dict(n=-1), dict(n=(1 << 30) + 1),
           dict(shard=-1), dict(shard=1), dict(shard=2, n_shards=2), dict(n_shards=0),
           dict(n=7), dict(n_shards=5, shard=4),                  # train: fewer images than batch * n_shards
           dict(dtype=2), dict(dtype=-1), dict(mode=2), dict(mode=-1),
           dict(out=C.c_void_p(got[0].data_ptr() + 2)), dict(step=C.c_void_p(step_t.data_ptr() + 1))]
  for bad in cases:
    a = dict(good, **bad)
    rc = lib.rigl_cifar_batch(*([a[k] for k in order] + [None]))
    assert rc == _lib.RIGL_EINVAL, bad
    assert b'rigl_cifar_batch' in lib.rigl_last_error(), bad
  assert lib.rigl_cifar_advance(None, None) == _lib.RIGL_EINVAL and b'rigl_cifar_advance' in lib.rigl_last_error()
  torch.cuda.synchronize()
  check('argument errors')
  for t in got:                                                  # the payloads still hold the sentinel: nothing ran
    assert bool((t.contiguous().view(torch.uint8) == R.SENTINEL).all())
  assert torch.equal(d_img, img0) and torch.equal(d_lab, lab0) and int(step_t) == 0
  # eval mode accepts a dataset smaller than a batch, and out_index may be NULL
  a = dict(good, mode=1, n=7, out_index=None)
  assert lib.rigl_cifar_batch(*([a[k] for k in order] + [C.c_void_p(torch.cuda.current_stream().cuda_stream)])) == _lib.RIGL_OK
  torch.cuda.synchronize()
  want = R.batch(_data(N)[0][:7], _data(N)[1][:7], B, 0, R.BF16, train=False)
  assert want[3] == 7 and bool((got[2] == int(R.sentinel_of(np.int32))).all())
  R.assert_same('eval n 7', (got[0], got[1], torch.from_numpy(np.concatenate([want[2], got[2].cpu().numpy()[7:]]))), want, B)
  with pytest.raises(_lib.RiglError) as ei:
    from rigl_amd import ops
    ops.cifar_batch(d_img, d_lab, 0, step_t, got[0], got[1])
  assert ei.value.code == _lib.RIGL_EINVAL and 'rigl_cifar_batch' in str(ei.value)
