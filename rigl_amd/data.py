"""The CIFAR input pipeline on the device (the reference's rigl/cifar_resnet/data_helper.py): the raw uint8 dataset lives in
HBM, and one HIP kernel per step (``ops.cifar_batch``) writes the standardized, mirror-padded, randomly cropped and flipped
batch -- in the epoch's keyed order -- straight into the buffers the model reads.  The step counter lives on the device, so a
captured graph that holds ``next_batch()`` replays fresh batches across epoch boundaries with no host work.

  DeviceCifar(images_u8, labels, batch, ...)   the loader; call ``next_batch()`` at the top of a GraphedStep's loss_fn
  load_cifar10_python(dir, split)              the standard cifar-10-batches-py pickles -> the two arrays DeviceCifar takes
  pad_input / preprocess_train                 host restatements on arrays, for parity reading (never on the training path)

The ImageNet image store (host side only; the reference constructs ``official.resnet.imagenet_input.ImageNetInput``, which it
does not vendor): DECODED uint8 RGB images of any size packed into one flat array with offsets / dims / labels tables -- the
format a device loader reads.  The device pipeline over it (crop, bicubic resize, flip, normalise) is specified bit for bit in
tests/imagenet_input_ref.py and not built yet; JPEG decoding happens once, on the host.

  pack_image_store / save_image_store / load_image_store   the store: flat uint8 + offsets / dims / labels tables
  image_store_from_folder(root, short_side)                decode (PIL) and short-side-resize a class/xxx.JPEG tree
  check_image_table(store_bytes, offsets, dims)            refuses a table row that does not lie inside the store
"""
import os
import pickle
import re

import numpy as np
import torch

from rigl_amd import ops
from rigl_amd.step_state import int32

IMG_SIZE = 32


class DeviceCifar(object):
  """Holds the dataset, the int32 step counter and fixed output buffers on ``device``.

  ``next_batch()`` enqueues the batch kernel, the widening of the labels to the int64 the loss kernel reads, and the counter's
  advance, and returns ``(images, labels)``: the SAME tensors every call ([batch, 32, 32, 3] of ``dtype``, int64 [batch]).
  Train: batch s of the keyed order (include/rigl_hip.h, rigl_cifar_batch); data parallel ranks pass their ``shard`` /
  ``n_shards`` and the same ``seed``.  Eval: the counter is the batch index; of the final partial batch only the first
  ``valid_count(b)`` slots are written."""

  def __init__(self, images_u8, labels, batch, train=True, seed=0, shard=0, n_shards=1, dtype=torch.bfloat16,
               device='cuda:0', with_indices=False):
    images_u8, labels = torch.as_tensor(images_u8), torch.as_tensor(labels)
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or tuple(images_u8.shape[1:]) != (IMG_SIZE, IMG_SIZE, 3):
      raise ValueError('images_u8 must be uint8 [N, 32, 32, 3] (HWC), got %s %s' % (images_u8.dtype, tuple(images_u8.shape)))
    if labels.numel() != images_u8.shape[0]:
      raise ValueError('%d labels for %d images' % (labels.numel(), images_u8.shape[0]))
    self.n, self.batch, self.train = int(images_u8.shape[0]), int(batch), bool(train)
    self.seed, self.shard, self.n_shards = int(seed), int(shard), int(n_shards)
    if self.batch <= 0 or not 0 <= self.shard < self.n_shards:
      raise ValueError('batch must be > 0 and shard in [0, n_shards)')
    if self.train and self.n < self.batch * self.n_shards:
      raise ValueError('train mode needs at least batch * n_shards = %d images, got %d' % (self.batch * self.n_shards, self.n))
    self.dataset_images = images_u8.to(device).contiguous()
    self.dataset_labels = labels.reshape(-1).to(device=device, dtype=torch.int32).contiguous()
    self.step = torch.zeros(1, dtype=torch.int32, device=device)
    self.images = torch.zeros(self.batch, IMG_SIZE, IMG_SIZE, 3, dtype=dtype, device=device)
    self.labels = torch.zeros(self.batch, dtype=torch.int64, device=device)
    self._labels32 = torch.zeros(self.batch, dtype=torch.int32, device=device)
    self._indices = torch.zeros(self.batch, dtype=torch.int32, device=device) if with_indices else None

  @property
  def steps_per_epoch(self):
    """Train: whole batches per pass (the order's tail is skipped); eval: batches, the final partial one included."""
    per = self.batch * self.n_shards
    return self.n // per if self.train else -(-self.n // per)

  def next_batch(self):
    ops.cifar_batch(self.dataset_images, self.dataset_labels, self.batch, self.step, self.images, self._labels32,
                    out_index=self._indices, train=self.train, seed0=self.seed, shard=self.shard, n_shards=self.n_shards)
    self.labels.copy_(self._labels32)
    ops.cifar_advance(self.step)
    return self.images, self.labels

  def valid_count(self, b):
    """Images the batch at counter value ``b`` writes (eval: the final batch may be partial, later ones are empty)."""
    if self.train:
      return self.batch
    first = (int(b) * self.n_shards + self.shard) * self.batch
    return max(0, min(self.batch, self.n - first))

  def position(self):
    """The counter, read back from the device (a synchronisation: for checkpoints, not for the training loop)."""
    return int(self.step.item())

  def seek(self, step):
    """Sets the counter (an upload: outside any graph capture).  Replays pick the new value up: they read the counter."""
    self.step.fill_(int32(step))

  def last_indices(self):
    """Dataset indices of the batch produced last (needs ``with_indices=True``)."""
    if self._indices is None:
      raise ValueError('DeviceCifar was built without with_indices=True')
    return self._indices


def load_cifar10_python(directory, split='train'):
  """(images uint8 [N, 32, 32, 3], labels int32 [N]) from a ``cifar-10-batches-py`` directory: ``data_batch_*`` (in numeric
  order) for 'train', ``test_batch`` for 'test' / 'eval'.  Each pickle holds planar rows (1024 R, 1024 G, 1024 B bytes);
  they are transposed to HWC.  Host-only; nothing is downloaded."""
  if not os.path.isdir(directory):
    raise FileNotFoundError('CIFAR-10 directory %r does not exist: unpack cifar-10-python.tar.gz and pass its '
                            'cifar-10-batches-py folder' % (directory,))
  if split == 'train':
    names = sorted((f for f in os.listdir(directory) if re.fullmatch(r'data_batch_\d+', f)), key=lambda f: int(f.rsplit('_', 1)[1]))
  elif split in ('test', 'eval'):
    names = [f for f in ('test_batch',) if os.path.exists(os.path.join(directory, f))]
  else:
    raise ValueError("split must be 'train', 'test' or 'eval', got %r" % (split,))
  if not names:
    raise FileNotFoundError('no %s batch in %r' % ('data_batch_* (train)' if split == 'train' else 'test_batch', directory))
  images, labels = [], []
  for name in names:
    with open(os.path.join(directory, name), 'rb') as f:
      d = pickle.load(f, encoding='bytes')
    data = np.asarray(d[b'data'], dtype=np.uint8).reshape(-1, 3, IMG_SIZE, IMG_SIZE)
    images.append(data.transpose(0, 2, 3, 1))
    labels.append(np.asarray(d[b'labels'], dtype=np.int32))
  return np.ascontiguousarray(np.concatenate(images)), np.concatenate(labels)


def pad_input(x, crop_dim=4):
  """[H, W, C] array with ``crop_dim`` mirrored border pixels on every side (the edge pixel repeats)."""
  return np.pad(np.asarray(x), ((crop_dim, crop_dim), (crop_dim, crop_dim), (0, 0)), mode='symmetric')


def preprocess_train(x, width, height, offset=None, flip=None, rng=np.random):
  """pad_input, a ``width`` x ``height`` crop at ``offset`` = (oy, ox), then a left-right flip; draws not given come from
  ``rng``.  The device pipeline takes its draws from the stateless Philox stream instead (include/rigl_hip.h)."""
  x = pad_input(x, 4)
  if offset is None:
    offset = (rng.randint(0, x.shape[0] - width + 1), rng.randint(0, x.shape[1] - height + 1))
  if flip is None:
    flip = rng.uniform() < 0.5
  x = x[offset[0]:offset[0] + width, offset[1]:offset[1] + height]
  return x[:, ::-1] if flip else x


def input_fn(params, **kw):
  """A DeviceCifar over ``params['data_directory']`` for ``params['data_split']`` ('train' or 'eval') at
  ``params['batch_size']``; further keywords go to DeviceCifar."""
  split = params['data_split']
  images, labels = load_cifar10_python(params['data_directory'], split)
  return DeviceCifar(images, labels, params['batch_size'], train=split == 'train', **kw)


# ---- the ImageNet image store ------------------------------------------------------------------------------------------
MAX_IMAGE_SIDE = 4096
STORE_FILES = ('store.u8', 'offsets.npy', 'dims.npy', 'labels.npy')


def pack_image_store(arrays, labels):
  """(store uint8 flat, offsets int64 [n], dims int32 [n, 2] = (h, w), labels int32 [n]) from a list of HWC uint8 RGB arrays:
  the images tightly packed one after the other (row stride 3 w, no alignment)."""
  arrays = [np.asarray(a) for a in arrays]
  labels = np.asarray(labels, dtype=np.int32).reshape(-1)
  if len(arrays) != labels.size:
    raise ValueError('%d labels for %d images' % (labels.size, len(arrays)))
  for j, a in enumerate(arrays):
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
      raise ValueError('image %d must be uint8 [h, w, 3] (HWC RGB), got %s %s' % (j, a.dtype, a.shape))
  dims = np.array([a.shape[:2] for a in arrays], dtype=np.int32).reshape(-1, 2)
  sizes = 3 * dims[:, 0].astype(np.int64) * dims[:, 1].astype(np.int64)
  offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64) if len(arrays) else np.zeros(0, np.int64)
  store = np.concatenate([a.reshape(-1) for a in arrays]) if len(arrays) else np.zeros(0, np.uint8)
  return store, offsets, dims, labels


def save_image_store(directory, store, offsets, dims, labels):
  """Writes the four files of a store: raw ``store.u8`` and ``offsets.npy`` / ``dims.npy`` / ``labels.npy``."""
  os.makedirs(directory, exist_ok=True)
  np.asarray(store, dtype=np.uint8).reshape(-1).tofile(os.path.join(directory, STORE_FILES[0]))
  np.save(os.path.join(directory, STORE_FILES[1]), np.asarray(offsets, dtype=np.int64).reshape(-1))
  np.save(os.path.join(directory, STORE_FILES[2]), np.asarray(dims, dtype=np.int32).reshape(-1, 2))
  np.save(os.path.join(directory, STORE_FILES[3]), np.asarray(labels, dtype=np.int32).reshape(-1))


def load_image_store(directory, mmap=True):
  """(store, offsets, dims, labels) as save_image_store wrote them; the store is an ``np.memmap`` (read-only) when ``mmap``."""
  for name in STORE_FILES:
    if not os.path.exists(os.path.join(directory, name)):
      raise FileNotFoundError('no %s in %r: an image store holds %s (save_image_store / image_store_from_folder)' % (
          name, directory, ', '.join(STORE_FILES)))
  path = os.path.join(directory, STORE_FILES[0])
  if os.path.getsize(path) == 0:
    store = np.zeros(0, np.uint8)
  else:
    store = np.memmap(path, dtype=np.uint8, mode='r') if mmap else np.fromfile(path, dtype=np.uint8)
  return (store,) + tuple(np.load(os.path.join(directory, n)) for n in STORE_FILES[1:])


def image_store_from_folder(root, short_side=None, extensions=('.jpeg', '.jpg', '.png')):
  """Decodes a ``root/<class>/<file>`` tree into a store (classes in sorted order are labels 0, 1, ...; files in sorted
  order).  With ``short_side`` every image is resized (PIL, bicubic) so that its shorter side has that length; that resize is a
  resolution trade made once on the host and not part of the pinned pipeline.  Host-only.  Returns pack_image_store's
  tuple plus the class names."""
  try:
    from PIL import Image  # pylint: disable=import-outside-toplevel
  except ImportError as e:
    raise ImportError('image_store_from_folder decodes with PIL (pillow), which is not installed; build the store on a '
                      'machine that has it, or pack decoded arrays with pack_image_store') from e
  classes = sorted(d for d in os.listdir(root) if os.path.isdir(os.path.join(root, d)))
  if not classes:
    raise FileNotFoundError('no class folder in %r' % (root,))
  arrays, labels = [], []
  for label, cls in enumerate(classes):
    for name in sorted(os.listdir(os.path.join(root, cls))):
      if not name.lower().endswith(tuple(extensions)):
        continue
      with Image.open(os.path.join(root, cls, name)) as im:
        im = im.convert('RGB')
        if short_side is not None and min(im.size) != int(short_side):
          k = float(short_side) / min(im.size)
          w, h = (max(1, int(round(v * k))) for v in im.size)
          im = im.resize((w, h), Image.BICUBIC)
        arrays.append(np.asarray(im, dtype=np.uint8))
      labels.append(label)
  return pack_image_store(arrays, labels) + (classes,)


def check_image_table(store_bytes, offsets, dims):
  """Raises ValueError naming the first row that does not describe an image inside the store: 1 <= h, w <= 4096,
  offset >= 0, offset + 3 h w <= store_bytes."""
  offsets, dims = np.asarray(offsets), np.asarray(dims)
  if offsets.ndim != 1 or dims.shape != (offsets.size, 2):
    raise ValueError('offsets must be [n] and dims [n, 2], got %s and %s' % (offsets.shape, dims.shape))
  off, h, w = offsets.astype(np.int64), dims[:, 0].astype(np.int64), dims[:, 1].astype(np.int64)
  side = (h >= 1) & (h <= MAX_IMAGE_SIDE) & (w >= 1) & (w <= MAX_IMAGE_SIDE)
  need = 3 * np.where(side, h * w, 0)
  bad = ~(side & (off >= 0) & (need <= store_bytes) & (off <= store_bytes - need))
  if bad.any():
    j = int(np.argmax(bad))
    raise ValueError('image table row %d is bad: h %d, w %d (must be 1 .. %d), offset %d, %d bytes needed of a store of %d' % (
        j, h[j], w[j], MAX_IMAGE_SIDE, off[j], 3 * h[j] * w[j], store_bytes))
