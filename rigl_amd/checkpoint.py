"""Exact training checkpoints: everything a run needs to carry on bit for bit, saved through ONE gather pass on the device.

  state = TrainingState(graph, optimizer, model=model, data=[loader], pruning=pruner, extra={'epoch': 3})
  state.save(path)                       # snapshot() + Snapshot.save(path)
  snap = state.snapshot()                # enqueues the gather and the copy-out, returns without a host synchronise
  ... training goes on ...
  snap.save(path)                        # waits for the copy-out only; writes path + '.tmp', then os.replace
                                         # (on a writer thread if you like: Snapshot's docstring says who owns the image when)
  extra = state.restore(path)            # or state.restore(snap): verifies everything first, then writes IN PLACE

``optimizer`` is what the training loop calls: a sparse wrapper (its ``_optimizer`` is the inner one) or an inner optimizer of
rigl_amd.train.  Constructing a TrainingState enqueues nothing: it finalizes the graph, makes the inner optimizer's slots
(``_ensure_slots``) and builds a table of named regions and a layout fingerprint.

STATE.  Device regions, in this order:
  graph/W, graph/BITS                               the master weights and the mask bitmap
  slot/momentum | slot/m, slot/v, adam/beta_powers  the inner optimizer's slot arenas (plain gradient descent has none)
  bn/<scope>/moving_mean, bn/<scope>/moving_variance   of every batch norm in graph.modules, in creation order
  dropout/step                                      where the model has a ``dropout_state``
  data/<i>/step                                     the counter of every DeviceCifar
  snfs/ema/<weights name>                           SparseMomentumOptimizer's gradient averages (made here, as zeros, where
                                                    the optimizer has not made them yet: it adopts them)
  pruning/thresholds                                gradual magnitude pruning's thresholds
Host scalars, in the file's JSON header: the global step, the sparse wrapper's ``_last_update_step``, PruningState's
``last_mask_update_step``, and ``extra``, the caller's own JSON-able dict (restore returns it).

NOT STATE, and why:
  G                          every step rewrites it before reading it
  the bf16 shadows           ``Graph.refresh_shadows`` rebuilds them from W and BITS (restore sets ``shadows_dirty``)
  accumulation arenas, workspaces   a MicroBatches sum lives inside one call (a snapshot while one is pending is refused)
  the learning-rate counter, the summaries' counter   StepCounters: they follow ``global_step`` by step_state's protocol and
                             find themselves stale after a restore, so the next call is an eager one that uploads them
  the summaries' ring        a log, not state: ``read()`` it before you restore
  the learning rate, the schedule   the caller's; neither saved nor checked
Random draws carry no state: every draw of a mask update, of dropout and of the input pipeline is keyed on (seed, counter).

FILE.  8 bytes magic ``RIGLCKP1`` | uint64 little-endian header length | the UTF-8 JSON header | zero bytes up to a multiple
of 256 | the packed image: region r at the running sum of the earlier regions' sizes, each rounded up to 256, zero bytes in
between.  The header holds the fingerprint, the host scalars, every region's name, size and digest (s1 = sum of its uint32
words, s2 = sum of (i + 1) * word i, both mod 2^64 -- an integrity check against truncation, misplacement and bit rot, not a
cryptographic one) and, as its last member ``~check``, the same digest of the header bytes in front of that member.  A file's
bytes depend on the state alone: saved twice, it is byte-identical.  A file moves between a GPU graph and a CPU graph.

RESTORE verifies, in this order, the header and the fingerprint, the file length, every region's digest recomputed on the host
in NumPy and the zero padding; only then it uploads the image and scatters it, and compares the digests the scatter computed
from what it wrote.  A failure raises CheckpointError naming the first difference; up to the upload nothing of the run has been
touched.  The scatter writes in place into the tensors the run already has and rebinds none, so the graphs a live GraphedStep
holds stay valid: a rollback costs one eager step, not a recapture.

Data parallel runs: every rank holds the same state; let rank 0 save.  Checkpoint averaging is out of scope.
"""
import copy
import io
import json
import os
import struct
import threading
import weakref

import numpy as np
import torch

from rigl_amd import ops
from rigl_amd import train
from rigl_amd.tf_checkpoint import CheckpointError

MAGIC = b'RIGLCKP1'
FORMAT_VERSION = 1
ALIGN = 256                      # _lib.STATE_ALIGN
_CHECK_KEY = b',"~check":['
_DIGEST_BLOCK = 1 << 20          # words per NumPy pass of the host digest
WRITE_BLOCK = 16 << 20           # bytes per write call of Snapshot.write


def _pad(n):
  return -(-int(n) // ALIGN) * ALIGN


def digest(words):
  """(s1, s2) of a uint32 array as Python ints: s1 = sum w_i, s2 = sum (i + 1) * w_i, both mod 2^64 (NumPy's uint64 arithmetic
  wraps as required)."""
  words = np.ascontiguousarray(words).view(np.uint32).reshape(-1)
  s1 = np.uint64(0)
  s2 = np.uint64(0)
  with np.errstate(over='ignore'):
    for b in range(0, words.size, _DIGEST_BLOCK):
      w = words[b:b + _DIGEST_BLOCK].astype(np.uint64)
      idx = np.arange(b + 1, b + 1 + w.size, dtype=np.uint64)
      s1 = s1 + w.sum(dtype=np.uint64)
      s2 = s2 + (w * idx).sum(dtype=np.uint64)
  return int(s1), int(s2)


def _bytes_digest(raw):
  """digest of a byte string: its length in front, zero bytes up to whole words."""
  buf = struct.pack('<Q', len(raw)) + raw + b'\0' * (-len(raw) % 4)
  return digest(np.frombuffer(buf, dtype=np.uint32))


def _offsets(sizes):
  out, off = [], 0
  for n in sizes:
    out.append(off)
    off += _pad(n)
  return out, off


def _encode_header(header):
  body = json.dumps(header, sort_keys=True, separators=(',', ':'), allow_nan=False).encode('utf-8')
  s1, s2 = _bytes_digest(body)
  return body[:-1] + _CHECK_KEY + b'%d,%d]}' % (s1, s2)


def _decode_header(raw):
  cut = raw.rfind(_CHECK_KEY)
  if cut < 0:
    raise CheckpointError('checkpoint header: no ~check member')
  try:
    header = json.loads(raw.decode('utf-8'))
    check = header.pop('~check')
    ok = [int(c) for c in check] == list(_bytes_digest(raw[:cut] + b'}')) and len(check) == 2
  except (ValueError, TypeError, KeyError, AttributeError) as e:
    raise CheckpointError('checkpoint header: not the JSON this format writes (%s)' % e) from None
  if not ok:
    raise CheckpointError('checkpoint header: its bytes do not match its ~check digest')
  return header


def _first_difference(want, got, path=''):
  """A line naming the first place two JSON-like values differ, or None."""
  if type(want) is not type(got):
    return '%s: the run has %r, the checkpoint %r' % (path or 'fingerprint', want, got)
  if isinstance(want, dict):
    for k in sorted(set(want) | set(got)):
      if k not in want or k not in got:
        return '%s/%s: only in the %s' % (path, k, 'run' if k in want else 'checkpoint')
      d = _first_difference(want[k], got[k], '%s/%s' % (path, k))
      if d:
        return d
    return None
  if isinstance(want, list):
    for i, (a, b) in enumerate(zip(want, got)):
      d = _first_difference(a, b, '%s[%d]' % (path, i))
      if d:
        return d
    if len(want) != len(got):
      return '%s: the run has %d entries, the checkpoint %d' % (path, len(want), len(got))
    return None
  return None if want == got else '%s: the run has %r, the checkpoint %r' % (path, want, got)


def _as_bytes(t):
  """A CPU tensor's bytes as a uint8 NumPy view."""
  return t.detach().contiguous().reshape(-1).view(torch.uint8).numpy()


class Snapshot:
  """One consistent image of a TrainingState, on its way to (or in) host memory.  ``save`` and a restore from it wait for the
  copy-out; the training stream never does.

  Ownership.  The image first lives in the TrainingState's ONE shared host buffer (pinned, on a GPU).  Every reader of that
  buffer -- ``write`` / ``save`` / ``tobytes`` here, ``TrainingState.restore(snapshot)`` -- holds this object's lock for the
  whole read, and the next ``TrainingState.snapshot()``, before it lets anything overwrite the buffer, takes the same lock
  and moves the image into memory of this object's own (``_own``): it waits for a save in flight on a writer thread, never
  tears it.  ``save`` then RELEASES the image (``keep=False``): the bytes are on disk, a later snapshot copies nothing, and a
  restore from this object raises (restore from the file).  ``save(path, keep=True)`` keeps it for a later rollback at the
  price of that host copy; a Snapshot that is dropped costs nothing either (the TrainingState holds it by weak reference)."""

  def __init__(self, header, packed, digests, done):
    self._header = header        # everything but the digests
    self._packed = packed        # uint8 NumPy view of the host image; None once released
    self._digests = digests      # int64 NumPy view [2n] (the uint64 bits), or a list of (s1, s2)
    self._done = done            # the copy-out's event, or None
    self._shared = True          # _packed / _digests are views of the TrainingState's shared buffers
    self._lock = threading.RLock()

  def wait(self):
    """Blocks until the copy-out has landed in host memory."""
    with self._lock:
      if self._done is not None:
        self._done.synchronize()
        self._done = None

  def _own(self):
    """The shared host buffers are about to be reused: waits for a reader in flight, then keeps a private copy."""
    with self._lock:
      if not self._shared or self._packed is None:
        return
      self.wait()
      self._digests = self.digests()
      self._packed = self._packed.copy()
      self._shared = False

  def release(self):
    """Lets go of the image: nothing of it is copied when the next snapshot is taken, and it can no longer be read."""
    with self._lock:
      self._packed = self._digests = self._done = None
      self._shared = False

  def _image(self):
    if self._packed is None:
      raise RuntimeError('this Snapshot was released (saved with keep=False): restore from the file it wrote')
    self.wait()
    return self._packed

  def digests(self):
    with self._lock:
      self._image()
      if isinstance(self._digests, list):
        return self._digests
      d = np.asarray(self._digests).view(np.uint64)
      return [(int(d[2 * i]), int(d[2 * i + 1])) for i in range(d.size // 2)]

  def header(self):
    """The file's header as a dict (waits for the copy-out: the digests are part of it)."""
    h = copy.deepcopy(self._header)
    h['regions'] = [[name, size, s1, s2] for (name, size), (s1, s2) in zip(h['regions'], self.digests())]
    return h

  def packed(self):
    """The packed image (a view: hold ``_lock`` while reading it where another thread may take the next snapshot)."""
    with self._lock:
      return self._image()

  def _head(self):
    """Magic, header length, header and the zero bytes up to the packed image."""
    raw = _encode_header(self.header())
    head = MAGIC + struct.pack('<Q', len(raw)) + raw
    return head + b'\0' * (-len(head) % ALIGN)

  def write(self, f):
    """The file's bytes into the binary file object ``f``, the image in blocks; the lock is held from the first byte to the
    last, so the shared buffer cannot be overwritten under it."""
    with self._lock:
      f.write(self._head())
      image = memoryview(self._image())
      for b in range(0, len(image), WRITE_BLOCK):
        f.write(image[b:b + WRITE_BLOCK])

  def tobytes(self):
    """The file's bytes."""
    out = io.BytesIO()
    self.write(out)
    return out.getvalue()

  def save(self, path, keep=False):
    """Writes ``path + '.tmp'``, then os.replace.  ``keep=False`` releases the image afterwards (see the class docstring)."""
    tmp = path + '.tmp'
    with self._lock:
      with open(tmp, 'wb') as f:
        self.write(f)
        f.flush()
        os.fsync(f.fileno())
      os.replace(tmp, path)
      if not keep:
        self.release()
    return path


def _parse(raw):
  """(header, packed uint8 view) of a file's bytes; checks the magic, the header, its padding and the length."""
  raw = np.frombuffer(raw, dtype=np.uint8) if not isinstance(raw, np.ndarray) else raw
  if raw.size < 16 or raw[:8].tobytes() != MAGIC:
    raise CheckpointError('not a training checkpoint: the file does not begin with %r' % MAGIC)
  hlen = struct.unpack('<Q', raw[8:16].tobytes())[0]
  if hlen > raw.size - 16:
    raise CheckpointError('checkpoint truncated: a header of %d bytes in a file of %d' % (hlen, raw.size))
  header = _decode_header(raw[16:16 + hlen].tobytes())
  data0 = _pad(16 + hlen)
  if raw.size < data0:
    raise CheckpointError('checkpoint truncated: %d bytes, the packed image begins at %d' % (raw.size, data0))
  if raw[16 + hlen:data0].any():
    raise CheckpointError('checkpoint header: the padding behind it is not zero')
  return header, raw[data0:]


class TrainingState:
  """See the module docstring."""

  def __init__(self, graph, optimizer, model=None, data=(), pruning=None, extra=None):
    from rigl_amd import sparse_optimizers as SO   # pylint: disable=import-outside-toplevel
    self._graph = graph
    self._outer = optimizer
    self._inner = inner = train.inner_optimizer(optimizer)
    self.extra = extra
    graph.finalize()
    if hasattr(inner, '_ensure_slots'):
      inner._ensure_slots()                        # pylint: disable=protected-access
    self._gs = graph.get_or_create_global_step()
    self._pruning = getattr(pruning, '_state', pruning)   # a pruning.Pruning, its PruningState, or None
    if hasattr(data, 'next_batch'):
      data = (data,)
    regions = [('graph/W', graph.W), ('graph/BITS', graph.BITS)]
    slots = list(inner.get_slot_names()) if hasattr(inner, 'get_slot_names') else []
    if slots == ['momentum']:
      regions.append(('slot/momentum', inner._slot))          # pylint: disable=protected-access
    elif slots == ['m', 'v']:
      regions += [('slot/m', inner._slot), ('slot/v', inner._slot_v), ('adam/beta_powers', inner._beta_powers)]   # pylint: disable=protected-access
    elif slots:
      raise NotImplementedError('TrainingState: an inner optimizer with the slots %r' % (slots,))
    for scope, mod in graph.modules.items():
      if hasattr(mod, 'moving_mean') and hasattr(mod, 'moving_variance'):
        regions += [('bn/%s/moving_mean' % scope, mod.moving_mean), ('bn/%s/moving_variance' % scope, mod.moving_variance)]
    if getattr(model, 'dropout_state', None) is not None:
      regions.append(('dropout/step', model.dropout_state.step))
    for i, d in enumerate(data):
      regions.append(('data/%d/step' % i, d.step))
    if isinstance(optimizer, SO.SparseMomentumOptimizer):
      for w in optimizer.get_weights():
        ema = optimizer._ema.get(w.name)             # pylint: disable=protected-access
        if ema is None:
          ema = optimizer._ema[w.name] = torch.zeros_like(w.grad)   # pylint: disable=protected-access
        regions.append(('snfs/ema/%s' % w.name, ema))
    if self._pruning is not None:
      regions.append(('pruning/thresholds', self._pruning.thresholds))
    for name, t in regions:
      if t.device != graph.W.device or not t.is_contiguous() or (t.numel() * t.element_size()) % 4:
        raise ValueError('TrainingState: region %s (%s on %s) is not a contiguous tensor of whole words on %s'
                         % (name, tuple(t.shape), t.device, graph.W.device))
    self._names = [n for n, _ in regions]
    self._tensors = [t for _, t in regions]
    self._sizes = [t.numel() * t.element_size() for t in self._tensors]
    self._offsets, self._packed_bytes = _offsets(self._sizes)
    self._on_gpu = graph.W.is_cuda
    self._arenas = (graph.W, graph.BITS)
    self.fingerprint = self._fingerprint(slots)
    # made by the first snapshot / restore (a construction enqueues nothing and allocates nothing on the device)
    self._table = self._staging = self._dev_digests = self._ws = None
    self._host = self._host_digests = self._host_t = self._host_digests_t = self._side = None
    self._copy_done = None       # the event behind the newest copy-out: the staging buffer is free once it has passed
    self._live = None            # weak reference to the Snapshot whose image is in the shared host buffers

  # ---- the layout ----------------------------------------------------------------------------------------------------------
  def _fingerprint(self, slots):
    from rigl_amd import variables as V   # pylint: disable=import-outside-toplevel
    g, inner, outer = self._graph, self._inner, self._outer
    hyper = {}
    for key in ('_momentum', '_nesterov', '_beta1', '_beta2', '_epsilon'):
      if getattr(inner, key, None) is not None:
        hyper[key.lstrip('_')] = getattr(inner, key)
    return {
        'format': FORMAT_VERSION,
        'variables': [[v.name, list(v.shape), int(v.kind), int(v.offset)] for v in g.variables.values()
                      if isinstance(v, V.Variable) and v.trainable],
        'masks': [m.name for m in g.get_masks()],
        'regions': [[n, s] for n, s in zip(self._names, self._sizes)],
        'optimizer': {'class': type(inner).__name__, 'slots': slots, 'hyper': hyper},
        'wrapper': type(outer).__name__ if outer is not inner else None,
    }

  def region_names(self):
    return list(self._names)

  def _check_layout(self):
    g = self._graph
    if g.W is not self._arenas[0] or g.BITS is not self._arenas[1]:
      raise RuntimeError('the graph was laid out again since this TrainingState was built: build a new one')

  def _check_quiet(self, what):
    if self._on_gpu and torch.cuda.is_current_stream_capturing():
      raise RuntimeError('TrainingState.%s during graph capture: a captured copy would replay a frozen image' % what)
    # a MicroBatches sum is pending: between its call and the LAST pass, or, under data parallelism, while its exchange is held
    # (passes 1..k-1) or handed the LAST pass (the k-th backward)
    acc = getattr(self._inner, 'accumulation', None)
    sync = getattr(self._inner, '_grad_sync', None)
    if (acc is not None and getattr(acc, '_pending', None) is not None) or getattr(sync, 'exchange_pending', False):
      raise RuntimeError('TrainingState.%s while the sum of a MicroBatches call is pending: finish the step first' % what)

  def _scalars(self):
    out = {'global_step': int(self._gs.value), 'last_update_step': None, 'pruning_last_mask_update_step': None}
    if hasattr(self._outer, '_last_update_step'):
      out['last_update_step'] = int(self._outer._last_update_step)   # pylint: disable=protected-access
    if self._pruning is not None:
      out['pruning_last_mask_update_step'] = int(self._pruning.last_mask_update_step)
    return out

  def _header(self):
    extra = json.loads(json.dumps(self.extra, allow_nan=False)) if self.extra is not None else None
    # (the fingerprint is shared, not copied: nothing writes to it, and Snapshot.header() hands out a copy)
    return {'fingerprint': self.fingerprint, 'scalars': self._scalars(), 'extra': extra,
            'regions': [[n, s] for n, s in zip(self._names, self._sizes)]}

  def _buffers(self):
    """The shared host image and, on a GPU, staging, digests, workspace and the side stream: made once."""
    n = len(self._tensors)
    if self._host is not None:
      return
    if not self._on_gpu:
      self._host, self._host_digests = np.zeros(self._packed_bytes, dtype=np.uint8), np.zeros(2 * n, dtype=np.int64)
      return
    dev = self._graph.W.device
    self._table = ops.state_table(self._tensors)
    assert ops.state_packed_bytes(self._table) == self._packed_bytes
    self._staging = torch.empty(max(self._packed_bytes, ALIGN), dtype=torch.uint8, device=dev)
    self._dev_digests = torch.empty(2 * n, dtype=torch.int64, device=dev)
    self._ws = torch.empty(max(ops.state_workspace_bytes(self._table), ALIGN), dtype=torch.uint8, device=dev)
    self._side = torch.cuda.Stream(device=dev)
    self._host_t = torch.empty(self._packed_bytes, dtype=torch.uint8).pin_memory()
    self._host_digests_t = torch.empty(2 * n, dtype=torch.int64).pin_memory()
    self._host, self._host_digests = self._host_t.numpy(), self._host_digests_t.numpy()   # (the views keep the tensors alive)

  def _free_host(self, but=None):
    """In front of anything that overwrites the shared host buffers: the Snapshot living there (unless it is ``but``) waits for
    its reader in flight and takes a private copy; one that was saved, released or dropped costs nothing."""
    live = self._live() if self._live is not None else None
    if live is not None and live is not but:
      live._own()                  # pylint: disable=protected-access
    if live is not but:
      self._live = None

  # ---- saving --------------------------------------------------------------------------------------------------------------
  def snapshot(self):
    """Enqueues the gather on the current stream and the copy-out on a side stream; returns a Snapshot without a host
    synchronise.  Refused (RuntimeError) during stream capture and while a MicroBatches sum is pending."""
    self._check_quiet('snapshot')
    self._check_layout()
    self._buffers()
    self._free_host()
    if not self._on_gpu:
      self._host[:] = 0
      d = self._host_digests.view(np.uint64)
      for i, (t, off, size) in enumerate(zip(self._tensors, self._offsets, self._sizes)):
        self._host[off:off + size] = _as_bytes(t)
        d[2 * i], d[2 * i + 1] = digest(self._host[off:off + size])
      done = None
    else:
      cur = torch.cuda.current_stream(self._graph.W.device)
      if self._copy_done is not None:
        cur.wait_event(self._copy_done)             # the staging buffer is read by the copy-out of the snapshot before
      ops.state_gather(self._table, self._staging, self._dev_digests, workspace_buffer=self._ws)
      gathered = torch.cuda.Event()
      gathered.record(cur)
      self._side.wait_event(gathered)
      with torch.cuda.stream(self._side):
        self._host_t.copy_(self._staging[:self._packed_bytes], non_blocking=True)
        self._host_digests_t.copy_(self._dev_digests, non_blocking=True)
        done = torch.cuda.Event()
        done.record(self._side)
      # allocated on the training stream, read on the side stream: the allocator must not hand the blocks out again (were this
      # object dropped now) before the copy-out has read them
      self._staging.record_stream(self._side)
      self._dev_digests.record_stream(self._side)
      self._copy_done = done
    # (the header is host work: behind the launches, so the device is busy meanwhile; the scalars do not move inside this call)
    snap = Snapshot(self._header(), self._host, self._host_digests, done)
    self._live = weakref.ref(snap)
    return snap

  def save(self, path):
    return self.snapshot().save(path)

  # ---- restoring -----------------------------------------------------------------------------------------------------------
  def restore(self, source):
    """``source``: a file's path or a Snapshot.  Verifies everything (module docstring), then writes the regions in place,
    sets the host scalars, ``graph.shadows_dirty`` and forgets the last backward pass.  Returns the checkpoint's ``extra``."""
    self._check_quiet('restore')
    self._check_layout()
    if isinstance(source, Snapshot):
      with source._lock:           # pylint: disable=protected-access  (its image may live in the shared buffer: read under its lock)
        return self._restore(source.header(), source.packed(), source)
    return self._restore(*_parse(np.fromfile(source, dtype=np.uint8)), None)

  def _restore(self, header, packed, source):
    try:
      fp, scalars, regions = header['fingerprint'], header['scalars'], header['regions']
      gs = int(scalars['global_step'])
      lus, pls = scalars['last_update_step'], scalars['pruning_last_mask_update_step']
    except (KeyError, TypeError, ValueError) as e:
      raise CheckpointError('checkpoint header: missing member (%s)' % e) from None
    diff = _first_difference(self.fingerprint, fp)
    if diff:
      raise CheckpointError('the checkpoint does not fit this run: %s' % diff)
    diff = _first_difference([[n, s] for n, s in zip(self._names, self._sizes)], [list(r[:2]) for r in regions], '/regions')
    if diff:
      raise CheckpointError('the checkpoint does not fit this run: %s' % diff)
    if packed.size != self._packed_bytes:
      raise CheckpointError('checkpoint %s: the packed image has %d bytes, the regions need %d'
                            % ('truncated' if packed.size < self._packed_bytes else 'too long', packed.size, self._packed_bytes))
    want = []
    for (name, size, s1, s2), off in zip(regions, self._offsets):
      got = digest(packed[off:off + size])
      if got != (int(s1), int(s2)):
        raise CheckpointError('region %s: the bytes have digest (%d, %d), the header says (%d, %d)' % ((name,) + got + (s1, s2)))
      if packed[off + size:off + _pad(size)].any():
        raise CheckpointError('region %s: the padding behind it is not zero' % name)
      want.append(got)
    # ---- everything checked: from here on the run is written ------------------------------------------------------------
    if self._on_gpu:
      self._buffers()
      cur = torch.cuda.current_stream(self._graph.W.device)
      if self._copy_done is not None:
        cur.wait_event(self._copy_done)
      self._staging[:self._packed_bytes].copy_(torch.from_numpy(packed))
      ops.state_scatter(self._table, self._staging, self._dev_digests, workspace_buffer=self._ws)
      d = self._dev_digests.cpu().numpy().view(np.uint64)
      for i, (name, (s1, s2)) in enumerate(zip(self._names, want)):
        if (int(d[2 * i]), int(d[2 * i + 1])) != (s1, s2):
          raise CheckpointError('region %s: the device wrote words of digest (%d, %d), the checkpoint holds (%d, %d)'
                                % (name, int(d[2 * i]), int(d[2 * i + 1]), s1, s2))
    else:
      for t, off, size in zip(self._tensors, self._offsets, self._sizes):
        src = torch.from_numpy(packed[off:off + size].copy()).view(t.dtype).reshape(t.shape)
        with torch.no_grad():
          t.copy_(src)
    self._gs.value = gs
    if lus is not None:
      self._outer._last_update_step = int(lus)     # pylint: disable=protected-access
    if pls is not None:
      self._pruning.last_mask_update_step.fill_(int(pls))
    self._graph.shadows_dirty = True
    if hasattr(self._inner, 'forget_backward'):
      self._inner.forget_backward()
    return header.get('extra')
