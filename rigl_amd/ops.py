"""Thin tensor-level wrappers over the C ABI (``include/rigl_hip.h``).

PyTorch is used for device memory and streams only: every function here takes
CUDA(=HIP) tensors, checks dtype/contiguity, and enqueues the hand-written
gfx950 kernels on ``torch.cuda.current_stream()``.  No function has a CPU or
PyTorch-op fallback; calling one without a GPU / without the built library
raises ``RiglError``.
"""
import ctypes as C
import os

import torch

from rigl_amd import _lib
from rigl_amd.step_state import int32 as _i32   # a Python int wrapped to int32 (TensorFlow's seeds, the step counters)
from rigl_amd._lib import (ConvDesc, PackLayer, PruneRegrowLayer,
                           PruneRegrowParams, RiglError, check)

_workspaces = {}


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)
_cur_device = getattr(torch._C, '_cuda_getDevice', None)


def _stream():
  """hipStream_t of torch's current stream on the current device (the raw-handle
  query is ~10x cheaper than building a torch.cuda.Stream object per launch)."""
  if _raw_stream is not None and _cur_device is not None:
    return C.c_void_p(_raw_stream(_cur_device()))
  return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
  return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _req(t, dtype, name, allow_none=False):
  if t is None:
    if allow_none:
      return
    raise ValueError('%s is None' % name)
  if not t.is_cuda:
    raise RiglError(_lib.RIGL_EINVAL,
                    '%s must live on the GPU (no CPU path exists)' % name)
  if t.dtype != dtype:
    raise TypeError('%s: expected %s, got %s' % (name, dtype, t.dtype))
  if not t.is_contiguous():
    raise ValueError('%s must be contiguous' % name)


# Bumped whenever a scratch buffer is (re)allocated: a captured HIP graph holds the OLD buffer's address, so
# train.GraphedStep drops its graphs when the generation it captured under is no longer current.
WORKSPACE_GENERATION = 0


def workspace(nbytes, device, tag=''):
  """Grow-only scratch buffer per device and user (stream-ordered reuse)."""
  global WORKSPACE_GENERATION
  key = (torch.device(device).index or 0, tag)
  ws = _workspaces.get(key)
  if ws is None or ws.numel() < nbytes:
    # grow geometrically (at most O(log) reallocations per user); the outgrown buffer is simply released -- kernels already
    # enqueued on it are safe (the caching allocator is stream-ordered) and train.GraphedStep compares WORKSPACE_GENERATION
    # before EVERY replay, so a captured graph never runs against a released buffer
    grown = max(int(nbytes), 1 << 20, (ws.numel() * 3 // 2) if ws is not None else 0)
    ws = torch.empty(grown, dtype=torch.uint8, device=device)
    _workspaces[key] = ws
    WORKSPACE_GENERATION += 1
  return ws


def n_mask_words(n):
  return (int(n) + 31) // 32


# ----------------------------------------------------------------------------
# mask bitmap
# ----------------------------------------------------------------------------
def mask_pack(mask01, out=None):
  """float 0/1 mask (any shape) -> int32 bitmap words (flat C order)."""
  _req(mask01, torch.float32, 'mask01')
  n = mask01.numel()
  if out is None:
    out = torch.zeros(n_mask_words(n), dtype=torch.int32, device=mask01.device)
  _req(out, torch.int32, 'bits')
  check(_lib.load().rigl_mask_pack(_ptr(mask01), _ptr(out), n, _stream()))
  return out


def mask_unpack(bits, shape):
  _req(bits, torch.int32, 'bits')
  out = torch.empty(shape, dtype=torch.float32, device=bits.device)
  check(_lib.load().rigl_mask_unpack(_ptr(bits), _ptr(out), out.numel(),
                                     _stream()))
  return out


# ----------------------------------------------------------------------------
# K2
# ----------------------------------------------------------------------------
_K2_OPTIONAL = ('momentum', 'dense_grad', 'drop_noise', 'score_drop', 'score_grow', 'grow_values')


def _prune_regrow_layer(slot, l, where=''):
  """Checks one prune / regrow layer dict and fills its PruneRegrowLayer ``slot``; returns (n, device, momentum2 or None)."""
  w, m2 = l.get('w'), l.get('momentum2')
  ref = w if w is not None else l['score_drop']
  n = ref.numel()
  for key in ('w', 'momentum2') + _K2_OPTIONAL:
    t = l.get(key)
    _req(t, torch.float32, key, allow_none=True)
    if t is not None and t.numel() != n:
      raise ValueError('%s%s has %d elements, expected %d' % (where, key, t.numel(), n))
    if key != 'momentum2':
      setattr(slot, key, t.data_ptr() if t is not None else None)
  _req(l['mask_bits'], torch.int32, 'mask_bits')
  if l['mask_bits'].numel() < n_mask_words(n):
    raise ValueError('%smask_bits too small' % where)
  slot.n = n
  slot.mask_bits = l['mask_bits'].data_ptr()
  return n, ref.device, m2


def _prune_regrow_params(drop_fraction, grow_init_mode, grow_init_div, momentum_reset_mode, initial_acc_scale, reinit_when_same):
  return PruneRegrowParams(float(drop_fraction), int(grow_init_mode), float(grow_init_div), int(momentum_reset_mode),
                           float(initial_acc_scale), int(bool(reinit_when_same)))


def prune_regrow(layers, drop_fraction, grow_init_mode=_lib.GROW_ZEROS,
                 grow_init_div=1.0, momentum_reset_mode=_lib.MOMRESET_GRAD,
                 initial_acc_scale=0.0, reinit_when_same=False):
  """Runs the fused prune/regrow update on a list of layers, in place.

  Each layer is a dict with tensors: ``w`` (fp32), ``mask_bits`` (int32),
  optional ``momentum``, ``momentum2``, ``dense_grad``, ``drop_noise``,
  ``score_drop``, ``score_grow``, ``grow_values`` (all fp32, same numel as
  ``w``).  ``momentum2`` is a second optimizer slot (Adam's v), reset like
  ``momentum``; only when some layer has one does the call go to
  rigl_prune_regrow_slots, otherwise it is rigl_prune_regrow.
  Returns an int32 tensor [n_layers, 8] of counts (see rigl_hip.h).
  """
  lib = _lib.load()
  nl = len(layers)
  if nl == 0:
    return torch.zeros((0, _lib.COUNTS_PER_LAYER), dtype=torch.int32)
  arr = (PruneRegrowLayer * nl)()
  ns = (C.c_int64 * nl)()
  mom2 = (C.c_void_p * nl)()
  for i, l in enumerate(layers):
    ns[i], dev, m2 = _prune_regrow_layer(arr[i], l, 'layer %d: ' % i)
    mom2[i] = m2.data_ptr() if m2 is not None else None
  prm = _prune_regrow_params(drop_fraction, grow_init_mode, grow_init_div, momentum_reset_mode, initial_acc_scale, reinit_when_same)
  ws = workspace(lib.rigl_prune_regrow_workspace_bytes(ns, nl), dev)
  counts = torch.zeros((nl, _lib.COUNTS_PER_LAYER), dtype=torch.int32,
                       device=dev)
  if any(l.get('momentum2') is not None for l in layers):
    check(lib.rigl_prune_regrow_slots(arr, mom2, nl, C.byref(prm), _ptr(counts), _ptr(ws),
                                      ws.numel(), _stream()))
  else:
    check(lib.rigl_prune_regrow(arr, nl, C.byref(prm), _ptr(counts), _ptr(ws),
                                ws.numel(), _stream()))
  return counts


def prune_regrow_selections(layer, drop_fraction, grow_init_mode=_lib.GROW_ZEROS, grow_init_div=1.0,
                            momentum_reset_mode=_lib.MOMRESET_GRAD, initial_acc_scale=0.0, reinit_when_same=False,
                            want_indices=True):
  """``prune_regrow`` on ONE layer (same dict), with the two selections read back (rigl_prune_regrow_selections): returns
  dict(counts int32[8], mask1_bits, mask2_bits (int32 bitmaps) and -- with ``want_indices`` -- idx1, idx2 int32[n]: the
  tensor's indices in tf.nn.top_k order of the drop / lifted grow score; the first counts[2] (n_keep) resp. counts[1]
  (n_prune) entries are the selected ones)."""
  lib = _lib.load()
  arr = PruneRegrowLayer()
  n, dev, m2 = _prune_regrow_layer(arr, layer)
  prm = _prune_regrow_params(drop_fraction, grow_init_mode, grow_init_div, momentum_reset_mode, initial_acc_scale, reinit_when_same)
  words = n_mask_words(n)
  out = dict(counts=torch.zeros(_lib.COUNTS_PER_LAYER, dtype=torch.int32, device=dev),
             mask1_bits=torch.zeros(words, dtype=torch.int32, device=dev),
             mask2_bits=torch.zeros(words, dtype=torch.int32, device=dev))
  if want_indices:
    out['idx1'] = torch.empty(n, dtype=torch.int32, device=dev)
    out['idx2'] = torch.empty(n, dtype=torch.int32, device=dev)
  ws = workspace(lib.rigl_prune_regrow_selections_workspace_bytes(n), dev, 'k2sel')
  check(lib.rigl_prune_regrow_selections_slots(C.byref(arr), _ptr(m2), C.byref(prm), _ptr(out['mask1_bits']),
                                               _ptr(out['mask2_bits']), _ptr(out.get('idx1')), _ptr(out.get('idx2')),
                                               _ptr(out['counts']), _ptr(ws), ws.numel(), _stream()))
  return out


def topk_mask(score, n_keep, out=None):
  """Bitmap of the n_keep largest scores (ties: lower flat index first)."""
  _req(score, torch.float32, 'score')
  n = score.numel()
  if out is None:
    out = torch.zeros(n_mask_words(n), dtype=torch.int32, device=score.device)
  lib = _lib.load()
  ns = (C.c_int64 * 1)(n)
  ws = workspace(lib.rigl_prune_regrow_workspace_bytes(ns, 1), score.device)
  check(lib.rigl_topk_mask(_ptr(score), n, int(n_keep), _ptr(out), _ptr(ws),
                           ws.numel(), _stream()))
  return out


def topk_mask_batched(items):
  """items: list of (score fp32 tensor, n_keep, mask_bits int32 tensor); all
  masks are rewritten in the same launches."""
  nl = len(items)
  if nl == 0:
    return
  lib = _lib.load()
  arr = (_lib.TopkLayer * nl)()
  ns = (C.c_int64 * nl)()
  for i, (score, n_keep, bits) in enumerate(items):
    _req(score, torch.float32, 'score')
    _req(bits, torch.int32, 'mask_bits')
    arr[i].score = score.data_ptr()
    arr[i].n = score.numel()
    arr[i].n_keep = int(n_keep)
    arr[i].mask_bits = bits.data_ptr()
    ns[i] = score.numel()
  ws = workspace(lib.rigl_prune_regrow_workspace_bytes(ns, nl), items[0][0].device)
  check(lib.rigl_topk_mask_batched(arr, nl, _ptr(ws), ws.numel(), _stream()))


def magnitude_prune_batched(items, threshold_decay=0.0, counts=None):
  """contrib model_pruning's mask update (rigl_magnitude_prune_batched) for many tensors in one call.

  items: list of (w fp32, mask_bits int32, threshold fp32 [1] device tensor, k) -- per tensor, the k-th largest |w|
  smoothed with the stored threshold (thr = cur * (1 - threshold_decay) + thr * threshold_decay, fp32) becomes the new
  threshold, and mask = |w| >= thr.  ``w`` is only read.  ``counts`` (optional int32 [len(items), 4] device tensor)
  receives n, k, new ones, old ones per tensor.  No host sync."""
  nl = len(items)
  if nl == 0:
    return counts
  lib = _lib.load()
  arr = (_lib.MagnitudePruneLayer * nl)()
  for i, (w, bits, thr, k) in enumerate(items):
    _req(w, torch.float32, 'w')
    _req(bits, torch.int32, 'mask_bits')
    _req(thr, torch.float32, 'threshold')
    n = w.numel()
    if bits.numel() < n_mask_words(n):
      raise ValueError('mask_bits too small')
    if thr.numel() != 1:
      raise ValueError('threshold must hold one float')
    arr[i].n = n
    arr[i].w = w.data_ptr()
    arr[i].mask_bits = bits.data_ptr()
    arr[i].threshold = thr.data_ptr()
    arr[i].k = int(k)
  if counts is not None:
    _req(counts, torch.int32, 'counts')
    if counts.numel() < nl * _lib.MAGPRUNE_COUNTS_PER_LAYER:
      raise ValueError('counts too small')
  ws = workspace(lib.rigl_magnitude_prune_batched_workspace_bytes(nl), items[0][0].device, 'magprune')
  check(lib.rigl_magnitude_prune_batched(arr, nl, float(threshold_decay), _ptr(counts), _ptr(ws), ws.numel(),
                                         _stream()))
  return counts


# ----------------------------------------------------------------------------
# K3
# ----------------------------------------------------------------------------
def _lr_device(lr, lr_device):
  """Exactly one of ``lr`` (a host number, a kernel argument) and ``lr_device`` (fp32 [1] on the GPU, read by the kernel)."""
  if (lr is None) == (lr_device is None):
    raise ValueError('pass exactly one of lr and lr_device')
  if lr_device is not None:
    _req(lr_device, torch.float32, 'lr_device')
    if lr_device.numel() != 1:
      raise ValueError('lr_device must hold 1 float')


def lr_kwargs(lr):
  """A rate held in one variable -- a host number or the fp32 [1] device tensor -- as the ``lr`` / ``lr_device`` argument."""
  return {'lr_device': lr} if torch.is_tensor(lr) else {'lr': lr}


def masked_sgd_momentum(w, grad, lr=None, momentum=None, mask_bits=None, mu=0.0,
                        weight_decay=0.0, grad_scale=1.0, nesterov=False,
                        w_shadow=None, lr_device=None):
  """K3 (rigl_masked_sgd_momentum).  ``lr_device`` (exclusive with ``lr``): the rate is read from that device tensor
  (rigl_masked_sgd_momentum_dlr), so a captured graph replays the value ``lr_schedule_step`` last wrote."""
  _lr_device(lr, lr_device)
  _req(w, torch.float32, 'w')
  _req(grad, torch.float32, 'grad')
  _req(momentum, torch.float32, 'momentum', allow_none=True)
  _req(mask_bits, torch.int32, 'mask_bits', allow_none=True)
  _req(w_shadow, torch.bfloat16, 'w_shadow', allow_none=True)
  n = w.numel()
  if grad.numel() != n or (momentum is not None and momentum.numel() != n):
    raise ValueError('size mismatch')
  if lr_device is not None:
    check(_lib.load().rigl_masked_sgd_momentum_dlr(
        n, _ptr(w), _ptr(momentum), _ptr(grad), _ptr(mask_bits), _ptr(lr_device),
        float(mu), float(weight_decay), float(grad_scale), int(bool(nesterov)),
        _ptr(w_shadow), _stream()))
    return
  check(_lib.load().rigl_masked_sgd_momentum(
      n, _ptr(w), _ptr(momentum), _ptr(grad), _ptr(mask_bits), float(lr),
      float(mu), float(weight_decay), float(grad_scale), int(bool(nesterov)),
      _ptr(w_shadow), _stream()))


def masked_adam(w, grad, m, v, beta_powers, lr=None, beta1=0.9, beta2=0.999, epsilon=1e-8, mask_bits=None,
                weight_decay=0.0, grad_scale=1.0, w_shadow=None, lr_device=None):
  """K3-Adam (rigl_masked_adam): one TF ApplyAdam step on w / m / v in place; the bias correction is read from the
  DEVICE tensor ``beta_powers`` (fp32 [2]), which ``adam_advance`` moves on once per step.  ``lr_device`` (exclusive with
  ``lr``): the rate is read from that device tensor as well (rigl_masked_adam_dlr)."""
  _lr_device(lr, lr_device)
  _req(w, torch.float32, 'w')
  _req(grad, torch.float32, 'grad')
  _req(m, torch.float32, 'm')
  _req(v, torch.float32, 'v')
  _req(beta_powers, torch.float32, 'beta_powers')
  _req(mask_bits, torch.int32, 'mask_bits', allow_none=True)
  _req(w_shadow, torch.bfloat16, 'w_shadow', allow_none=True)
  n = w.numel()
  if grad.numel() != n or m.numel() != n or v.numel() != n or beta_powers.numel() != 2:
    raise ValueError('size mismatch')
  if mask_bits is not None and mask_bits.numel() < n_mask_words(n):
    raise ValueError('mask_bits too small')
  if w_shadow is not None and w_shadow.numel() != n:
    raise ValueError('w_shadow size mismatch')
  if lr_device is not None:
    check(_lib.load().rigl_masked_adam_dlr(
        n, _ptr(w), _ptr(m), _ptr(v), _ptr(grad), _ptr(mask_bits), _ptr(beta_powers), _ptr(lr_device), float(beta1),
        float(beta2), float(epsilon), float(weight_decay), float(grad_scale), _ptr(w_shadow), _stream()))
    return
  check(_lib.load().rigl_masked_adam(
      n, _ptr(w), _ptr(m), _ptr(v), _ptr(grad), _ptr(mask_bits), _ptr(beta_powers), float(lr), float(beta1),
      float(beta2), float(epsilon), float(weight_decay), float(grad_scale), _ptr(w_shadow), _stream()))


def adam_advance(beta_powers, beta1=0.9, beta2=0.999):
  """beta_powers *= (beta1, beta2) on the device (AdamOptimizer._finish)."""
  _req(beta_powers, torch.float32, 'beta_powers')
  if beta_powers.numel() != 2:
    raise ValueError('beta_powers must hold 2 floats')
  check(_lib.load().rigl_adam_advance(_ptr(beta_powers), float(beta1), float(beta2), _stream()))


def lr_schedule_step(sched, step, lr_out):
  """lr_out[0] = sched(step[0]); step[0] += 1, on the device (rigl_lr_schedule_step).  ``sched``: an _lib.LrSchedule (what
  schedules.Schedule.descriptor() returns), ``step``: int32 [1], ``lr_out``: fp32 [1]."""
  if not isinstance(sched, _lib.LrSchedule):
    raise TypeError('sched: expected an LrSchedule descriptor, got %s' % type(sched).__name__)
  _req(step, torch.int32, 'step')
  _req(lr_out, torch.float32, 'lr_out')
  if step.numel() != 1 or lr_out.numel() != 1:
    raise ValueError('step and lr_out must hold 1 element each')
  check(_lib.load().rigl_lr_schedule_step(C.byref(sched), _ptr(step), _ptr(lr_out), _stream()))


def summary_table(entries):
  """The host table of rigl_summary_step: ``entries`` is a list of (w fp32 [n], g fp32 [n], mask_bits int32 | None,
  weight_decay, apply_mask).  The table holds raw pointers: the caller keeps the tensors alive."""
  arr = (_lib.SummaryEntry * max(len(entries), 1))()
  for i, (w, g, bits, wd, apply_mask) in enumerate(entries):
    _req(w, torch.float32, 'w')
    _req(g, torch.float32, 'g')
    _req(bits, torch.int32, 'mask_bits', allow_none=True)
    if g.numel() != w.numel():
      raise ValueError('summary_table: entry %d: w has %d elements, g %d' % (i, w.numel(), g.numel()))
    if bits is not None and bits.numel() < n_mask_words(w.numel()):
      raise ValueError('summary_table: entry %d: mask_bits too small' % i)
    arr[i].n = w.numel()
    arr[i].w = w.data_ptr()
    arr[i].g = g.data_ptr()
    arr[i].mask_bits = bits.data_ptr() if bits is not None else None
    arr[i].weight_decay = float(wd)
    arr[i].apply_mask = int(bool(apply_mask))
  return arr, len(entries)


def summary_slot_bytes(n_entries):
  return int(_lib.load().rigl_summary_slot_bytes(int(n_entries)))


def summary_workspace_bytes(table):
  arr, n = table
  return int(_lib.load().rigl_summary_workspace_bytes(arr, n))


def summary_step(table, step, ring, ring_slots, grad_scale=1.0, loss=None, lr=None, lr_device=None, max_blocks=0):
  """One record of the training summaries (rigl_summary_step): the sums and counts of every entry of ``table``
  (summary_table) into slot ``step[0] % ring_slots`` of ``ring`` (uint8, ring_slots * summary_slot_bytes), then
  ``step[0] += 1``.  ``loss``: fp32 device scalar or None; the rate is ``lr_device`` (fp32 [1] on the GPU) or the float ``lr``.
  Enqueues kernels only (capture-safe); the scratch comes from ops.workspace."""
  arr, n = table
  _lr_device(lr, lr_device)
  _req(step, torch.int32, 'step')
  _req(ring, torch.uint8, 'ring')
  _req(loss, torch.float32, 'loss', allow_none=True)
  if step.numel() != 1 or (loss is not None and loss.numel() != 1):
    raise ValueError('step and loss must hold 1 element each')
  lib = _lib.load()
  if ring_slots < 1 or ring.numel() < ring_slots * lib.rigl_summary_slot_bytes(n):
    raise ValueError('ring of %d bytes is too small for %d slots of %d entries' % (ring.numel(), ring_slots, n))
  need = lib.rigl_summary_workspace_bytes(arr, n)
  ws = workspace(need, ring.device, 'summary')
  check(lib.rigl_summary_step(arr, n, float(grad_scale), _ptr(loss), _ptr(lr_device), float(lr if lr is not None else 0.0),
                              _ptr(step), _ptr(ring), int(ring_slots), _ptr(ws), ws.numel(), int(max_blocks), _stream()))


def grad_accumulate(acc, grad, mode, loss=None, loss_acc=None, loss_mean=None, inv_k=1.0, max_blocks=0):
  """One pass of micro-batch gradient accumulation over two fp32 arenas of one size (rigl_grad_accumulate).  ``mode``:
  _lib.ACC_FIRST ``acc = grad``, ACC_ADD ``acc += grad``, ACC_LAST ``grad = acc + grad`` (acc is only read).  ``loss`` (fp32 [1]
  on the GPU, or None: no loss arithmetic): FIRST ``loss_acc = loss``, ADD ``loss_acc += loss``, LAST ``loss_mean =
  (loss_acc + loss) * inv_k``.  One launch, capture-safe."""
  _req(acc, torch.float32, 'acc')
  _req(grad, torch.float32, 'grad')
  _req(loss, torch.float32, 'loss', allow_none=True)
  _req(loss_acc, torch.float32, 'loss_acc', allow_none=True)
  _req(loss_mean, torch.float32, 'loss_mean', allow_none=True)
  if acc.numel() != grad.numel():
    raise ValueError('size mismatch: acc has %d elements, grad %d' % (acc.numel(), grad.numel()))
  for t, name in ((loss, 'loss'), (loss_acc, 'loss_acc'), (loss_mean, 'loss_mean')):
    if t is not None and t.numel() != 1:
      raise ValueError('%s must hold 1 float' % name)
  check(_lib.load().rigl_grad_accumulate(acc.numel(), _ptr(acc), _ptr(grad), int(mode), _ptr(loss), _ptr(loss_acc),
                                         _ptr(loss_mean), float(inv_k), int(max_blocks), _stream()))


def grad_accumulate_ranges(acc, grad, ranges, mode, loss=None, loss_acc=None, loss_mean=None, inv_k=1.0, max_blocks=0):
  """grad_accumulate over ``ranges`` of the two arenas only, in one launch (rigl_grad_accumulate_ranges): a sequence of up to
  _lib.ACC_MAX_RANGES ``(offset, length)`` pairs in elements, ascending and not overlapping, every offset a multiple of 4, a
  length arbitrary (0 is legal).  Nothing outside the ranges is read or written.  The loss arithmetic of ``mode`` is done once
  per launch, with an empty ``ranges`` too.  One launch, capture-safe."""
  _req(acc, torch.float32, 'acc')
  _req(grad, torch.float32, 'grad')
  _req(loss, torch.float32, 'loss', allow_none=True)
  _req(loss_acc, torch.float32, 'loss_acc', allow_none=True)
  _req(loss_mean, torch.float32, 'loss_mean', allow_none=True)
  if acc.numel() != grad.numel():
    raise ValueError('size mismatch: acc has %d elements, grad %d' % (acc.numel(), grad.numel()))
  for t, name in ((loss, 'loss'), (loss_acc, 'loss_acc'), (loss_mean, 'loss_mean')):
    if t is not None and t.numel() != 1:
      raise ValueError('%s must hold 1 float' % name)
  ranges = list(ranges)
  arr = (_lib.AccRange * max(len(ranges), 1))()
  for i, (off, length) in enumerate(ranges):
    arr[i].offset, arr[i].length = int(off), int(length)
  check(_lib.load().rigl_grad_accumulate_ranges(acc.numel(), _ptr(acc), _ptr(grad), arr, len(ranges), int(mode), _ptr(loss),
                                                _ptr(loss_acc), _ptr(loss_mean), float(inv_k), int(max_blocks), _stream()))


def state_table(tensors):
  """The host table of rigl_state_gather / rigl_state_scatter: one region per tensor (contiguous, on one GPU, a whole number
  of 4-byte words).  The table holds raw pointers: the caller keeps the tensors alive."""
  arr = (_lib.StateRegion * max(len(tensors), 1))()
  for i, t in enumerate(tensors):
    if not t.is_cuda:
      raise RiglError(_lib.RIGL_EINVAL, 'state_table: region %d must live on the GPU (no CPU path exists)' % i)
    if not t.is_contiguous():
      raise ValueError('state_table: region %d must be contiguous' % i)
    nbytes = t.numel() * t.element_size()
    if nbytes % 4:
      raise ValueError('state_table: region %d has %d bytes, no multiple of 4' % (i, nbytes))
    arr[i].ptr = t.data_ptr() if nbytes else None
    arr[i].bytes = nbytes
  return arr, len(tensors)


def state_packed_bytes(table):
  arr, n = table
  return int(_lib.load().rigl_state_packed_bytes(arr, n))


def state_workspace_bytes(table):
  arr, n = table
  return int(_lib.load().rigl_state_workspace_bytes(arr, n))


def _state_move(fn, table, packed, digests, max_blocks, ws):
  arr, n = table
  _req(packed, torch.uint8, 'packed')
  _req(digests, torch.int64, 'digests')
  lib = _lib.load()
  if packed.numel() < lib.rigl_state_packed_bytes(arr, n):
    raise ValueError('packed holds %d bytes, the table needs %d' % (packed.numel(), lib.rigl_state_packed_bytes(arr, n)))
  if digests.numel() < 2 * n:
    raise ValueError('digests holds %d words, the table needs %d' % (digests.numel(), 2 * n))
  need = lib.rigl_state_workspace_bytes(arr, n)
  if ws is None:
    ws = workspace(need, packed.device, 'state')
  else:
    _req(ws, torch.uint8, 'workspace')
  check(getattr(lib, fn)(arr, n, _ptr(packed), _ptr(digests), _ptr(ws), ws.numel(), int(max_blocks), _stream()))


def state_gather(table, packed, digests, max_blocks=0, workspace_buffer=None):
  """The regions of ``table`` (state_table) into ``packed`` (uint8, 256-byte aligned, state_packed_bytes): region r at the
  running sum of the earlier sizes, each rounded up to 256, zero bytes in between; ``digests`` (int64 [2n], the uint64 sums'
  bits) gets (s1, s2) of every region from the words read (rigl_state_gather).  Kernels only; the scratch is ``workspace_buffer`` (uint8, state_workspace_bytes) or ops.workspace."""
  _state_move('rigl_state_gather', table, packed, digests, max_blocks, workspace_buffer)


def state_scatter(table, packed, digests, max_blocks=0, workspace_buffer=None):
  """``packed`` back into the regions of ``table``, in place; ``digests`` gets (s1, s2) of every region from the words written
  (rigl_state_scatter).  The padding of ``packed`` is not read and nothing outside a region is written."""
  _state_move('rigl_state_scatter', table, packed, digests, max_blocks, workspace_buffer)


def pack_weights_batched(layers):
  """layers: list of (w fp32 [k*cout], mask_bits|None, k, cout, hwio|None,
  ohwi|None)."""
  nl = len(layers)
  if nl == 0:
    return
  arr = (PackLayer * nl)()
  for i, (w, bits, k, cout, hwio, ohwi) in enumerate(layers):
    _req(w, torch.float32, 'w')
    _req(bits, torch.int32, 'mask_bits', allow_none=True)
    _req(hwio, torch.bfloat16, 'hwio', allow_none=True)
    _req(ohwi, torch.bfloat16, 'ohwi', allow_none=True)
    if w.numel() != k * cout:
      raise ValueError('pack_weights: w has %d elements, k*cout=%d' %
                       (w.numel(), k * cout))
    arr[i].w = w.data_ptr()
    arr[i].mask_bits = bits.data_ptr() if bits is not None else None
    arr[i].hwio = hwio.data_ptr() if hwio is not None else None
    arr[i].ohwi = ohwi.data_ptr() if ohwi is not None else None
    arr[i].k = k
    arr[i].cout = cout
  check(_lib.load().rigl_pack_weights_batched(arr, nl, _stream()))


def pack_weights(w, mask_bits, k, cout, hwio=None, ohwi=None):
  pack_weights_batched([(w, mask_bits, k, cout, hwio, ohwi)])


# ----------------------------------------------------------------------------
# K1
# ----------------------------------------------------------------------------
# Dense-equivalent work of the K1 / K1d calls, counted on the host while ``work_count(True)`` is set: the
# algorithmic FLOPs / bytes that bench.py's roofline divides by the kernels' measured time.
WORK = {'fwd_macs': 0, 'dgrad_macs': 0, 'wgrad_macs': 0, 'depthwise_bytes': 0}
_work_on = False


def work_count(on=True):
  global _work_on
  _work_on = bool(on)
  if on:
    for k in WORK:
      WORK[k] = 0


def _count_macs(kind, d):
  if _work_on:
    WORK[kind] += d.n * d.ho * d.wo * d.kh * d.kw * d.cin * d.cout


def _count_depthwise(d):
  if _work_on:      # one bf16 tensor read + one written (fwd, dgrad) or two read (wgrad); weights are negligible
    WORK['depthwise_bytes'] += 2 * d.n * (d.h * d.w + d.ho * d.wo) * d.cin


# Plan-dependent sizes (workspace bytes, statistics parts) are asked of the library once per descriptor AND per knob
# generation: the C-side answers follow the run-time knobs (a kernel switched on after a layer's first call changes how
# many partial rows its forward writes; a stale, larger count would leave batch norm summing uninitialised rows).
# The generation is the LIBRARY's (rigl_tune_generation): a knob flipped through any other binding of the same process
# invalidates the cache too.


_GEN_WORD = None      # the library's counter, read in place (a ctypes call per lookup cost the launch-bound wrn22 step 0.5 ms)


def _plan_cached(d, name, fn):
  global _GEN_WORD
  if _GEN_WORD is None:
    _GEN_WORD = C.c_uint64.from_address(_lib.load().rigl_tune_generation_addr())
  gen = _GEN_WORD.value
  c = getattr(d, '_plan', None)
  if c is None or c[0] != gen:
    c = (gen, {})
    d._plan = c
  v = c[1].get(name)
  if v is None:
    v = c[1][name] = fn()
  return v


def conv_desc(n, h, w, cin, cout, kh, kw, stride, pad_top, pad_left, ho, wo):
  sh, sw = (stride, stride) if isinstance(stride, int) else stride
  return ConvDesc(n, h, w, cin, ho, wo, cout, kh, kw, sh, sw, pad_top,
                  pad_left)


def mfma_supported(d):
  """Shapes the implicit-GEMM MFMA kernels take (else the direct kernels)."""
  return d.cout % 8 == 0


def mfma_dgrad_supported(d):
  return d.cout % 8 == 0 and d.cin % 8 == 0


def conv_fwd(d, x, w_ohwi, y=None, force_ref=False, stats=False, *, scale_shift=None, residual=None, relu=False, part=None):
  """y[N,Ho,Wo,Cout] (bf16, NHWC memory) = conv(x, w).  With ``stats`` returns
  (y, partials): fp32 [parts, 2, Cout] batch-norm partial sums of y left by the
  conv epilogue (None where the MFMA path does not apply).
  Eval: with ``scale_shift`` (fp32 [2, Cout], bn_infer_params) y = bf16(relu?(fmaf(conv, scale, shift) (+ residual))), the frozen
  batch norm in the forward's epilogue where the layer takes it (conv_fwd_takes_bn_epilogue), else the plain forward followed by
  bn_apply -- the same bits either way.
  ``part`` (optional, with ``stats``): the caller's fp32 [rigl_conv2d_stats_parts, 2, Cout] buffer for the partials."""
  if scale_shift is not None or residual is not None or relu:
    if scale_shift is None or stats or force_ref:
      raise ValueError('conv_fwd: residual / relu need scale_shift, and the eval epilogue leaves no statistics')
    return _conv_fwd_infer(d, x, None, w_ohwi, scale_shift, residual, relu, y)
  _req(x, torch.bfloat16, 'x')
  _req(w_ohwi, torch.bfloat16, 'w_ohwi')
  _count_macs('fwd_macs', d)
  y = _out(y, (d.n, d.ho, d.wo, d.cout), torch.bfloat16, x.device, 'y')
  lib = _lib.load()
  if force_ref or not mfma_supported(d):
    check(lib.rigl_conv2d_fwd_ref(C.byref(d), _ptr(x), _ptr(w_ohwi), _ptr(y),
                                  _stream()))
    return (y, None) if stats else y
  need = _plan_cached(d, 'ws_fwd', lambda: lib.rigl_conv2d_workspace_bytes(C.byref(d), 0))
  d._stats_parts = _plan_cached(d, 'stats_parts', lambda: lib.rigl_conv2d_stats_parts(C.byref(d)))
  ws = workspace(need, x.device) if need else None
  if stats:
    part = _stats_out(part, d._stats_parts, d.cout, x.device)
  else:
    part = None
  check(lib.rigl_masked_conv2d_fwd_stats(
      C.byref(d), _ptr(x), _ptr(w_ohwi), _ptr(y), _ptr(part),
      part.numel() if part is not None else 0, _ptr(ws),
      ws.numel() if ws is not None else 0, _stream()))
  return (y, part) if stats else y


def _stats_out(part, parts, c, device):
  """The statistics buffer of a forward: the caller's (checked: fp32, exactly [parts, 2, c]) or a fresh one."""
  if part is None:
    return torch.empty((parts, 2, c), dtype=torch.float32, device=device)
  _req(part, torch.float32, 'part')
  if tuple(part.shape) != (parts, 2, c):
    raise ValueError('part must be [%d, 2, %d]' % (parts, c))
  return part


def _out(t, shape, dtype, device, name):
  """An output tensor: the caller's (checked: dtype, contiguous, the element count of ``shape``) or a fresh one."""
  if t is None:
    return torch.empty(shape, dtype=dtype, device=device)
  _req(t, dtype, name)
  n = 1
  for s in shape:
    n *= s
  if t.numel() != n:
    raise ValueError('%s must hold %d elements (%s)' % (name, n, 'x'.join(map(str, shape))))
  return t


def conv_fwd_takes_bn_input(d):
  """Does this layer's forward take the batch norm in front of it on its operand load (rigl_conv2d_fwd_takes_bn_input)?"""
  if not mfma_supported(d):
    return False
  return bool(_plan_cached(d, 'fwd_bn_input', lambda: int(_lib.load().rigl_conv2d_fwd_takes_bn_input(C.byref(d)))))


def conv_fwd_bnrelu(d, x_pre, saved, w_ohwi, a_out, y=None, stats=False, *, scale_shift=None, residual=None, relu=False, part=None):
  """y = conv(relu(bn(x_pre)), w) with the batch norm's apply pass on the operand load (rigl_masked_conv2d_fwd_bnrelu):
  ``saved`` = fp32 [4, Cin] (mean, invstd, scale, shift: bn_statistics), ``a_out`` (bf16, the shape of x_pre) receives
  relu(bn(x_pre)) as a side output.  Returns y or (y, partials) like conv_fwd.
  Eval (``a_out`` None): ``saved`` may be [2, Cin] (bn_infer_params), no side output is written, and ``scale_shift`` /
  ``residual`` / ``relu`` add the frozen batch norm behind the conv as conv_fwd does; where the layer does not take the
  transform (conv_fwd_takes_bn_epilogue(d, bn_on_load=True)) bn_apply runs first -- the same bits."""
  if a_out is None:
    if stats:
      raise ValueError('conv_fwd_bnrelu: the eval form leaves no statistics')
    if scale_shift is None and (residual is not None or relu):
      raise ValueError('conv_fwd_bnrelu: residual / relu need scale_shift')
    return _conv_fwd_infer(d, x_pre, saved, w_ohwi, scale_shift, residual, relu, y)
  if scale_shift is not None or residual is not None or relu:
    raise ValueError('conv_fwd_bnrelu: the epilogue arguments belong to the eval form (a_out None)')
  _req(x_pre, torch.bfloat16, 'x_pre')
  _req(a_out, torch.bfloat16, 'a_out')
  _req(w_ohwi, torch.bfloat16, 'w_ohwi')
  _req(saved, torch.float32, 'saved')
  if saved.numel() != 4 * d.cin or a_out.numel() != x_pre.numel() or x_pre.numel() != d.n * d.h * d.w * d.cin:
    raise ValueError('saved must be [4, Cin]; x_pre and a_out [n, h, w, Cin]')
  _count_macs('fwd_macs', d)
  y = _out(y, (d.n, d.ho, d.wo, d.cout), torch.bfloat16, x_pre.device, 'y')
  lib = _lib.load()
  if stats:
    parts = _plan_cached(d, 'stats_parts', lambda: lib.rigl_conv2d_stats_parts(C.byref(d)))
    part = _stats_out(part, parts, d.cout, x_pre.device)
  else:
    part = None
  check(lib.rigl_masked_conv2d_fwd_bnrelu(C.byref(d), _ptr(x_pre), _ptr(saved[2]), _ptr(a_out), _ptr(w_ohwi), _ptr(y), _ptr(part),
                                          part.numel() if part is not None else 0, None, 0, _stream()))
  return (y, part) if stats else y


def conv_fwd_takes_bn_epilogue(d, bn_on_load=False, residual=False):
  """Does this layer's eval forward take the frozen batch norm (+ a residual) in its epilogue (and, with ``bn_on_load``, the one
  in front on its operand load) -- rigl_conv2d_fwd_takes_bn_epilogue; knob "eval_fuse" 0 says no for every layer."""
  if not mfma_supported(d):
    return False
  a, r = int(bool(bn_on_load)), int(bool(residual))
  return bool(_plan_cached(d, 'fwd_bn_epilogue%d%d' % (a, r),
                           lambda: int(_lib.load().rigl_conv2d_fwd_takes_bn_epilogue(C.byref(d), a, r))))


def _conv_fwd_infer(d, x, in_ss, w_ohwi, ss, residual, relu, y):
  """conv(a, w) [-> frozen batch norm (+ residual) (+ ReLU)], a = x or bf16(relu(bn_in(x))) with in_ss = [.., 2, Cin] rows of
  scale / shift: fused where legal, else the separate passes."""
  _req(x, torch.bfloat16, 'x')
  _req(w_ohwi, torch.bfloat16, 'w_ohwi')
  for t, nm, c in ((in_ss, 'in_scale_shift', d.cin), (ss, 'scale_shift', d.cout)):
    if t is not None:
      _req(t, torch.float32, nm)
      if t.dim() != 2 or t.shape[0] not in (2, 4) or t.shape[1] != c:
        raise ValueError('%s must be [2, %d] (or a [4, %d] saved block)' % (nm, c, c))
  if x.numel() != d.n * d.h * d.w * d.cin:
    raise ValueError('x must be [n, h, w, Cin] of the descriptor')
  _req(residual, torch.bfloat16, 'residual', allow_none=True)
  if residual is not None and residual.numel() != d.n * d.ho * d.wo * d.cout:
    raise ValueError('residual must have the shape of the output')
  y = _out(y, (d.n, d.ho, d.wo, d.cout), torch.bfloat16, x.device, 'y')
  if conv_fwd_takes_bn_epilogue(d, in_ss is not None, residual is not None):
    _count_macs('fwd_macs', d)
    check(_lib.load().rigl_masked_conv2d_fwd_bn_infer(
        C.byref(d), _ptr(x), _ptr(in_ss[-2] if in_ss is not None else None), _ptr(w_ohwi),
        _ptr(ss[-2] if ss is not None else None), _ptr(residual), int(bool(relu)), _ptr(y), _stream()))
    return y
  if in_ss is not None:
    x = bn_apply(x, in_ss, relu=True)
    if ss is not None and conv_fwd_takes_bn_epilogue(d, False, residual is not None):
      return _conv_fwd_infer(d, x, None, w_ohwi, ss, residual, relu, y)
  if ss is None:
    return conv_fwd(d, x, w_ohwi, y)
  return bn_apply(conv_fwd(d, x, w_ohwi), ss, relu=relu, residual=residual, y=y)


def conv_dgrad(d, dy, w_hwio, dx=None, force_ref=False, addend=None):
  """dx = conv2d_backprop_input(dy, w) (+ addend, fused into the epilogue: the
  gradient accumulation of a tensor that feeds this conv and a shortcut)."""
  _count_macs('dgrad_macs', d)
  _req(dy, torch.bfloat16, 'dy')
  _req(w_hwio, torch.bfloat16, 'w_hwio')
  dx = _out(dx, (d.n, d.h, d.w, d.cin), torch.bfloat16, dy.device, 'dx')
  if addend is not None:
    _req(addend, torch.bfloat16, 'addend')
    if addend.numel() != dx.numel():
      raise ValueError('addend must have the shape of dx')
  lib = _lib.load()
  if force_ref or not mfma_dgrad_supported(d):
    check(lib.rigl_conv2d_dgrad_ref(C.byref(d), _ptr(dy), _ptr(w_hwio),
                                    _ptr(dx), _stream()))
    if addend is not None:
      dx += addend.view_as(dx)
    return dx
  check(lib.rigl_masked_conv2d_dgrad_acc(C.byref(d), _ptr(dy), _ptr(w_hwio),
                                         _ptr(addend), _ptr(dx), None, 0,
                                         _stream()))
  return dx


def conv_wgrad(d, x, dy, dw=None, force_ref=False):
  """Dense fp32 dW in HWIO order (flat [kh*kw*cin*cout])."""
  _count_macs('wgrad_macs', d)
  _req(x, torch.bfloat16, 'x')
  _req(dy, torch.bfloat16, 'dy')
  dw = _out(dw, (d.kh * d.kw * d.cin * d.cout,), torch.float32, x.device, 'dw')
  lib = _lib.load()
  if force_ref or not mfma_supported(d):
    check(lib.rigl_conv2d_wgrad_ref(C.byref(d), _ptr(x), _ptr(dy), _ptr(dw),
                                    _stream()))
    return dw
  need = _plan_cached(d, 'ws_wgrad', lambda: lib.rigl_conv2d_workspace_bytes(C.byref(d), 2))
  ws = workspace(need, x.device) if need else None
  check(lib.rigl_masked_conv2d_wgrad(C.byref(d), _ptr(x), _ptr(dy), _ptr(dw),
                                     _ptr(ws),
                                     ws.numel() if ws is not None else 0,
                                     _stream()))
  return dw


def conv_bwd_takes_masked_addend(d):
  """Should the producer of this layer's addend hand it over unmasked + a 1-bit mask (rigl_masked_conv2d_bwd_masked) instead
  of writing the masked copy?  (rigl_conv2d_bwd_takes_masked_addend: the layers whose default selection has the masked form.)"""
  return bool(_plan_cached(d, 'masked_addend', lambda: int(_lib.load().rigl_conv2d_bwd_takes_masked_addend(C.byref(d)))))


def conv_bwd_takes_bn_apply(d):
  """Does this layer's one-call backward apply the backward of the batch norm BEHIND it on its dY load
  (rigl_masked_conv2d_bwd_bnapply)?  Knob "bn_bwd_on_load" (RIGL_BN_BWD_ON_LOAD) 0 says no for every layer."""
  if not (mfma_supported(d) and mfma_dgrad_supported(d)):
    return False
  return bool(_plan_cached(d, 'bwd_bn_apply', lambda: int(_lib.load().rigl_conv2d_bwd_takes_bn_apply(C.byref(d)))))


def _conv_bwd(d, x, dy, w_hwio, dw, dx, on_dw_ready, launch, need_dx=True, dx_shape=None, dgrad_desc=None, f32=False):
  """The one host transition every one-call conv backward shares: operand checks, the wgrad / dgrad MAC counts, the cached
  weight-gradient workspace, dX (the caller's, checked, or a fresh one; None without ``need_dx``), ``launch(lib, dx pointer,
  workspace pointer, workspace bytes)`` -- the form's own C entry point -- and ``on_dw_ready`` once dW's last kernel is enqueued.
  ``dx_shape`` / ``dgrad_desc``: where dX is not [n, h, w, cin] of ``d``.  ``f32``: the fp32 twin's dtypes and workspace."""
  act = torch.float32 if f32 else torch.bfloat16
  _req(x, act, 'x')
  _req(dy, act, 'dy')
  _req(dw, torch.float32, 'dw')
  lib = _lib.load()
  _count_macs('wgrad_macs', d)
  if f32:
    need = _plan_cached(d, 'ws_wgrad_f32', lambda: lib.rigl_conv2d_wgrad_f32_workspace_bytes(C.byref(d)))
  else:
    need = _plan_cached(d, 'ws_wgrad', lambda: lib.rigl_conv2d_workspace_bytes(C.byref(d), 2))
  ws = workspace(need, x.device, 'wg32' if f32 else 'wg') if need else None
  if need_dx:
    _req(w_hwio, act, 'w_hwio')
    _count_macs('dgrad_macs', dgrad_desc if dgrad_desc is not None else d)
    dx = _out(dx, dx_shape or (d.n, d.h, d.w, d.cin), act, dy.device, 'dx')
  else:
    dx = None
  check(launch(lib, _ptr(dx), _ptr(ws), ws.numel() if ws is not None else 0))
  if on_dw_ready is not None:
    on_dw_ready()
  return dx


def conv_bwd_bnapply(d, x, dout, w_hwio, dw, y, relu_bits, saved, coef, addend=None, on_dw_ready=None, dx=None):
  """conv_bwd of the conv in front of a batch norm whose backward apply pass was not run (bn_bwd_reduce): ``dout`` is the
  gradient w.r.t. relu(bn(y) + shortcut), ``y`` this conv's forward output, ``relu_bits`` / ``saved`` the batch norm's forward
  products, ``coef`` bn_bwd_reduce's.  dW into ``dw``; returns dX (+ ``addend``) -- the bits of bn_bwd followed by conv_bwd."""
  if not conv_bwd_takes_bn_apply(d):
    raise ValueError('this layer\'s backward does not take the batch-norm apply (conv_bwd_takes_bn_apply)')
  _req(dout, torch.bfloat16, 'dout')
  _req(y, torch.bfloat16, 'y')
  _req(addend, torch.bfloat16, 'addend', allow_none=True)
  _req(saved, torch.float32, 'saved'); _req(coef, torch.float32, 'coef')
  _req(relu_bits, torch.uint8, 'relu_bits')
  n_out = d.n * d.ho * d.wo * d.cout
  if dout.numel() != n_out or y.numel() != n_out or relu_bits.numel() * 8 != n_out:
    raise ValueError('dout and y must have the shape of the conv output and relu_bits one bit per element of it')
  if saved.numel() != 4 * d.cout or coef.numel() != 3 * d.cout:
    raise ValueError('saved must be [4, Cout] and coef [3, Cout]')
  if addend is not None and addend.numel() != d.n * d.h * d.w * d.cin:
    raise ValueError('addend must have the shape of dx')
  return _conv_bwd(d, x, dout, w_hwio, dw, dx, on_dw_ready, lambda lib, pdx, ws, nws: lib.rigl_masked_conv2d_bwd_bnapply(
      C.byref(d), _ptr(x), _ptr(dout), _ptr(w_hwio), _ptr(addend), _ptr(dw), pdx, ws, nws, _ptr(y), _ptr(relu_bits),
      _ptr(saved[0]), _ptr(saved[1]), _ptr(coef), _stream()))


def conv_bwd(d, x, dy, w_hwio, dw, need_dx=True, addend=None, on_dw_ready=None, addend_sub=None, addend_bits=None,
             dx=None):
  """dW (into ``dw``, dense fp32) and -- when ``need_dx`` -- dX (+ ``addend``) of one conv with a single host
  transition and, for ordinary layers, a single launch (rigl_masked_conv2d_bwd) followed by the split-K reduce that
  completes dW.  ``on_dw_ready`` is called once dW's last kernel has been enqueued (the data-parallel exchange launches
  its buckets from there).  Returns dX or None.
  ``addend_sub`` = (sh, sw): ``addend`` is the gradient of the subsampled view x[:, ::sh, ::sw, :] -- bf16
  [n, ceil(h / sh), ceil(w / sw), cin] -- added at those pixels only (rigl_masked_conv2d_bwd_sub).
  ``addend_bits`` (uint8, one bit per element of ``addend``): the addend counts only where its bit is set
  (rigl_masked_conv2d_bwd_masked; a layer whose kernels have no masked form is refused by the library: RiglError).
  ``dx`` (optional, with ``need_dx``): the caller's bf16 [n, h, w, cin] tensor for dX instead of a fresh one."""
  if addend_sub is not None and tuple(addend_sub) == (1, 1):
    addend_sub = None
  n_in = d.n * d.h * d.w * d.cin
  if addend_bits is not None:
    if addend is None or not need_dx or addend_sub is not None:
      raise ValueError('addend_bits needs an addend and dX, and does not combine with addend_sub')
    _req(addend, torch.bfloat16, 'addend'); _req(addend_bits, torch.uint8, 'addend_bits')
    if addend.numel() != n_in or addend_bits.numel() * 8 != n_in:
      raise ValueError('addend must have the shape of dx and addend_bits one bit per element of it')
    return _conv_bwd(d, x, dy, w_hwio, dw, dx, on_dw_ready, lambda lib, pdx, ws, nws: lib.rigl_masked_conv2d_bwd_masked(
        C.byref(d), _ptr(x), _ptr(dy), _ptr(w_hwio), _ptr(addend), _ptr(addend_bits), _ptr(dw), pdx, ws, nws, _stream()))
  if addend_sub is not None:
    if addend is None or not need_dx:
      raise ValueError('addend_sub needs an addend and dX')
    if not (mfma_supported(d) and mfma_dgrad_supported(d)):
      raise ValueError('addend_sub needs cin % 8 == cout % 8 == 0')
  if not (mfma_supported(d) and (not need_dx or mfma_dgrad_supported(d))):
    conv_wgrad(d, x, dy, dw)
    if on_dw_ready is not None:
      on_dw_ready()
    return conv_dgrad(d, dy, w_hwio, dx=dx, addend=addend) if need_dx else None
  _req(addend, torch.bfloat16, 'addend', allow_none=True)
  if addend_sub is not None:
    sh, sw = addend_sub
    if addend.numel() != d.n * (-(-d.h // sh)) * (-(-d.w // sw)) * d.cin:
      raise ValueError('addend must be [n, ceil(h / sh), ceil(w / sw), cin]')
    return _conv_bwd(d, x, dy, w_hwio, dw, dx, on_dw_ready, lambda lib, pdx, ws, nws: lib.rigl_masked_conv2d_bwd_sub(
        C.byref(d), _ptr(x), _ptr(dy), _ptr(w_hwio), _ptr(addend), int(sh), int(sw), _ptr(dw), pdx, ws, nws, _stream()))
  if need_dx and addend is not None and addend.numel() != n_in:
    raise ValueError('addend must have the shape of dx')
  return _conv_bwd(d, x, dy, w_hwio, dw, dx, on_dw_ready, lambda lib, pdx, ws, nws: lib.rigl_masked_conv2d_bwd(
      C.byref(d), _ptr(x), _ptr(dy), _ptr(w_hwio), _ptr(addend), _ptr(dw), pdx, ws, nws, _stream()), need_dx=need_dx)


def conv_bwd_grid(d, x, dy, w_hwio, dw, on_dw_ready=None, dx=None):
  """Backward of a strided 1x1 conv without padding with dX on the conv's own grid: returns bf16 [n, ho, wo, cin] -- the
  gradient at the pixels the conv read (zero elsewhere, never materialised) -- and writes the dense dW
  (rigl_masked_conv2d_bwd_grid).  The consumer is conv_bwd(..., addend=that, addend_sub=strides) of the tensor's other
  reader."""
  grid = ConvDesc(d.n, d.ho, d.wo, d.cin, d.ho, d.wo, d.cout, 1, 1, 1, 1, 0, 0)      # (the stride-1 conv the dgrad amounts to)
  return _conv_bwd(d, x, dy, w_hwio, dw, dx, on_dw_ready, lambda lib, pdx, ws, nws: lib.rigl_masked_conv2d_bwd_grid(
      C.byref(d), _ptr(x), _ptr(dy), _ptr(w_hwio), _ptr(dw), pdx, ws, nws, _stream()),
                   dx_shape=(d.n, d.ho, d.wo, d.cin), dgrad_desc=grid)


# ----------------------------------------------------------------------------
# K1 in fp32 arithmetic (validation twin; the reference's --precision=float32)
# ----------------------------------------------------------------------------
# ----------------------------------------------------------------------------
# masked conv + ReLU without a batch norm (VGG)
# ----------------------------------------------------------------------------
def conv_fwd_takes_relu_epilogue(d):
  """Does this layer's forward body carry the ReLU epilogue (rigl_conv2d_fwd_takes_relu_epilogue)?  Else conv_fwd_relu runs the
  plain forward and the stand-alone relu pass -- the same bits."""
  return bool(_plan_cached(d, 'fwd_relu_epi', lambda: int(_lib.load().rigl_conv2d_fwd_takes_relu_epilogue(C.byref(d)))))


def conv_bwd_takes_relu_epilogue(d):
  """Does this layer's dgrad body carry the ReLU gate (rigl_conv2d_bwd_takes_relu_epilogue)?"""
  return bool(_plan_cached(d, 'bwd_relu_epi', lambda: int(_lib.load().rigl_conv2d_bwd_takes_relu_epilogue(C.byref(d)))))


def conv_fwd_relu(d, x, w_ohwi, y=None):
  """y = bf16(max(conv(x, w), 0)) (rigl_masked_conv2d_fwd_relu): the pre-activation is never stored."""
  _req(x, torch.bfloat16, 'x')
  _req(w_ohwi, torch.bfloat16, 'w_ohwi')
  if x.numel() != d.n * d.h * d.w * d.cin:
    raise ValueError('x must be [n, h, w, Cin] of the descriptor')
  _count_macs('fwd_macs', d)
  y = _out(y, (d.n, d.ho, d.wo, d.cout), torch.bfloat16, x.device, 'y')
  lib = _lib.load()
  need = _plan_cached(d, 'ws_fwd', lambda: lib.rigl_conv2d_workspace_bytes(C.byref(d), 0))
  ws = workspace(need, x.device) if need else None
  check(lib.rigl_masked_conv2d_fwd_relu(C.byref(d), _ptr(x), _ptr(w_ohwi), _ptr(y), _ptr(ws),
                                        ws.numel() if ws is not None else 0, _stream()))
  return y


def conv_bwd_relu(d, x, dy, w_hwio, dw, on_dw_ready=None, dx=None):
  """dW (dense fp32, into ``dw``) and dX = bf16(dgrad(dy)) * [x > 0] of a conv whose input ``x`` is a ReLU output (or a max
  pool of one) -- rigl_masked_conv2d_bwd_relu.  ``dy`` must already carry this conv's own ReLU gate.  Returns dX."""
  _req(x, torch.bfloat16, 'x')
  _req(dy, torch.bfloat16, 'dy')
  if x.numel() != d.n * d.h * d.w * d.cin or dy.numel() != d.n * d.ho * d.wo * d.cout:
    raise ValueError('x / dy must have the shapes of the descriptor')
  return _conv_bwd(d, x, dy, w_hwio, dw, dx, on_dw_ready, lambda lib, pdx, ws, nws: lib.rigl_masked_conv2d_bwd_relu(
      C.byref(d), _ptr(x), _ptr(dy), _ptr(w_hwio), _ptr(dw), pdx, ws, nws, _stream()))


def relu_fwd(x, y=None):
  """Stand-alone y = relu(x) on a bf16 tensor (rigl_relu_fwd; ``y`` may be ``x``)."""
  _req(x, torch.bfloat16, 'x')
  if y is None:
    y = torch.empty_like(x)
  _req(y, torch.bfloat16, 'y')
  if y.numel() != x.numel():
    raise ValueError('y must have the shape of x')
  check(_lib.load().rigl_relu_fwd(x.numel(), _ptr(x), _ptr(y), _stream()))
  return y


def relu_bwd(dy, x, dx=None):
  """Stand-alone dx = dy * [x > 0] on bf16 tensors (rigl_relu_bwd; ``dx`` may be ``dy``)."""
  _req(dy, torch.bfloat16, 'dy')
  _req(x, torch.bfloat16, 'x')
  if dx is None:
    dx = torch.empty_like(dy)
  _req(dx, torch.bfloat16, 'dx')
  if not dy.numel() == x.numel() == dx.numel():
    raise ValueError('dy, x and dx must have one shape')
  check(_lib.load().rigl_relu_bwd(dy.numel(), _ptr(dy), _ptr(x), _ptr(dx), _stream()))
  return dx


def conv_fwd_f32(d, x, w_hwio, mask_bits=None, y=None):
  """y[N,Ho,Wo,Cout] fp32 = conv(x, mask * W): fp32 NHWC activations, the fp32 master weights (flat HWIO) and the
  mask bitmap (None: dense), on the fp32 MFMA (rigl_masked_conv2d_fwd_f32)."""
  _req(x, torch.float32, 'x')
  _req(w_hwio, torch.float32, 'w_hwio')
  _req(mask_bits, torch.int32, 'mask_bits', allow_none=True)
  _count_macs('fwd_macs', d)
  if y is None:
    y = torch.empty((d.n, d.ho, d.wo, d.cout), dtype=torch.float32, device=x.device)
  _req(y, torch.float32, 'y')
  check(_lib.load().rigl_masked_conv2d_fwd_f32(C.byref(d), _ptr(x), _ptr(w_hwio), _ptr(mask_bits), _ptr(y), _stream()))
  return y


def conv_bwd_f32(d, x, dy, w_hwio, mask_bits, dw, need_dx=True, addend=None, on_dw_ready=None, dx=None):
  """fp32 twin of conv_bwd: dense dW (fp32 HWIO, overwritten) and -- when ``need_dx`` -- dX (+ ``addend``)."""
  _req(addend, torch.float32, 'addend', allow_none=True)
  _req(mask_bits, torch.int32, 'mask_bits', allow_none=True)
  if need_dx and addend is not None and addend.numel() != d.n * d.h * d.w * d.cin:
    raise ValueError('addend must have the shape of dx')
  dx = _conv_bwd(d, x, dy, w_hwio, dw, dx, on_dw_ready, lambda lib, pdx, ws, nws: lib.rigl_masked_conv2d_wgrad_f32(
      C.byref(d), _ptr(x), _ptr(dy), _ptr(dw), ws, nws, _stream()), need_dx=need_dx, f32=True)
  if need_dx:       # (dW is complete and announced; the fp32 dgrad is a launch of its own)
    check(_lib.load().rigl_masked_conv2d_dgrad_f32(C.byref(d), _ptr(dy), _ptr(w_hwio), _ptr(mask_bits), _ptr(addend), _ptr(dx),
                                                   _stream()))
  return dx


# ----------------------------------------------------------------------------
# K1d depthwise
# ----------------------------------------------------------------------------
def depthwise_fwd(d, x, w, stats=False, y=None, part=None):
  """y = depthwise conv(x, w).  With ``stats`` returns (y, partials): fp32 [parts, 2, C] batch-norm partial sums of y left
  by the kernel's epilogue (None for shapes without one).  ``y`` / ``part`` (optional): the caller's output tensors."""
  _count_depthwise(d)
  _req(x, torch.bfloat16, 'x')
  _req(w, torch.float32, 'w')
  y = _out(y, (d.n, d.ho, d.wo, d.cout), torch.bfloat16, x.device, 'y')
  lib = _lib.load()
  if stats:
    parts = _plan_cached(d, 'dw_parts', lambda: int(lib.rigl_depthwise_conv2d_stats_parts(C.byref(d))))
    if parts > 0:
      part = _stats_out(part, parts, d.cout, x.device)
      check(lib.rigl_depthwise_conv2d_fwd_stats(C.byref(d), _ptr(x), _ptr(w), _ptr(y), _ptr(part), part.numel(), _stream()))
      return y, part
  check(lib.rigl_depthwise_conv2d_fwd(C.byref(d), _ptr(x), _ptr(w), _ptr(y), _stream()))
  return (y, None) if stats else y


def depthwise_dgrad(d, dy, w, dx=None):
  _count_depthwise(d)
  _req(dy, torch.bfloat16, 'dy')
  _req(w, torch.float32, 'w')
  dx = _out(dx, (d.n, d.h, d.w, d.cin), torch.bfloat16, dy.device, 'dx')
  check(_lib.load().rigl_depthwise_conv2d_dgrad(C.byref(d), _ptr(dy), _ptr(w), _ptr(dx), _stream()))
  return dx


def depthwise_wgrad(d, x, dy, dw):
  _count_depthwise(d)
  _req(x, torch.bfloat16, 'x')
  _req(dy, torch.bfloat16, 'dy')
  _req(dw, torch.float32, 'dw')
  lib = _lib.load()
  ws = workspace(lib.rigl_depthwise_conv2d_workspace_bytes(C.byref(d)), x.device)
  check(lib.rigl_depthwise_conv2d_wgrad(C.byref(d), _ptr(x), _ptr(dy), _ptr(dw), _ptr(ws), ws.numel(), _stream()))
  return dw


# ----------------------------------------------------------------------------
# fused batch-norm (+ residual) (+ ReLU)
# ----------------------------------------------------------------------------
def _bn_plan(x, partials=None):
  """(rows, channels, workspace or None, parts) of a batch-norm call over the channel axis of bf16 ``x``: ``partials`` (checked:
  fp32 [parts, 2, C]) stand in for the statistics pass, so the reduction workspace is only fetched without them."""
  _req(x, torch.bfloat16, 'x')
  c = x.shape[-1]
  m = x.numel() // c
  parts = 0
  if partials is not None:
    _req(partials, torch.float32, 'partials')
    if partials.dim() != 3 or partials.shape[1] != 2 or partials.shape[2] != c:
      raise ValueError('partials must be [parts, 2, %d]' % c)
    parts = partials.shape[0]
  ws = workspace(_lib.load().rigl_bn_workspace_bytes(m, c), x.device) if partials is None else None
  return m, c, ws, parts


def bn_fwd(x, gamma, beta, running_mean, running_var, momentum, eps, relu,
           residual=None, partials=None, want_relu_bits=False):
  """x [..., C] bf16 contiguous.  Returns (y, saved) with saved = fp32 [4, C]
  (mean, invstd, scale, shift).  ``partials`` (fp32 [parts, 2, C], from
  conv_fwd(stats=True)) replaces the statistics pass over x.  With
  ``want_relu_bits`` returns (y, saved, bits): uint8 [numel/8], bit j of byte i =
  (y[8i+j] > 0), the ReLU mask the backward needs instead of y."""
  _req(residual, torch.bfloat16, 'residual', allow_none=True)
  for t, nm in ((gamma, 'gamma'), (beta, 'beta')):
    _req(t, torch.float32, nm)
  m, c, ws, parts = _bn_plan(x, partials)
  y = torch.empty_like(x)
  saved = torch.empty((4, c), dtype=torch.float32, device=x.device)
  bits = torch.empty(x.numel() // 8, dtype=torch.uint8, device=x.device) \
      if (want_relu_bits and relu) else None
  check(_lib.load().rigl_bn_fwd_stats(
      m, c, _ptr(x), _ptr(residual), _ptr(gamma), _ptr(beta),
      _ptr(running_mean), _ptr(running_var), float(momentum), float(eps),
      int(bool(relu)), _ptr(y), _ptr(saved[0]), _ptr(saved[1]), _ptr(saved[2]),
      _ptr(saved[3]), _ptr(partials), parts, _ptr(bits), _ptr(ws),
      ws.numel() if ws is not None else 0, _stream()))
  return (y, saved, bits) if want_relu_bits else (y, saved)


def bn_bwd(x, y, dy, gamma, saved, relu, dgamma, dbeta, want_dres=False,
           relu_bits=None):
  """Returns (dx, dres|None); dgamma / dbeta (fp32 [C]) are overwritten.  The
  ReLU mask comes from ``relu_bits`` (bn_fwd(want_relu_bits=True)), else ``y``,
  else it is recomputed from x."""
  _req(relu_bits, torch.uint8, 'relu_bits', allow_none=True)
  _req(dy, torch.bfloat16, 'dy')
  _req(y, torch.bfloat16, 'y', allow_none=True)
  m, c, ws, _ = _bn_plan(x)
  dx = torch.empty_like(x)
  dres = torch.empty_like(x) if want_dres else None
  check(_lib.load().rigl_bn_bwd(m, c, _ptr(x), _ptr(y), _ptr(relu_bits), _ptr(dy), _ptr(gamma),
                                _ptr(saved[0]), _ptr(saved[1]), _ptr(saved[2]),
                                _ptr(saved[3]), int(bool(relu)), _ptr(dx), _ptr(dres),
                                _ptr(dgamma), _ptr(dbeta), _ptr(ws), ws.numel(), _stream()))
  return dx, dres


def bn_bwd_reduce(x, dy, gamma, saved, relu, relu_bits, dgamma, dbeta):
  """bn_bwd without its apply pass (rigl_bn_bwd_reduce): dgamma / dbeta (fp32 [C]) are overwritten; returns coef, fp32 [3, C]
  (a = gamma * invstd, b = mean dz, c = mean dz * xhat), for conv_bwd_bnapply of the conv that produced ``x``."""
  _req(dy, torch.bfloat16, 'dy')
  _req(relu_bits, torch.uint8, 'relu_bits', allow_none=not relu)
  m, c, ws, _ = _bn_plan(x)
  if dy.numel() != x.numel() or (relu and relu_bits.numel() * 8 != x.numel()):
    raise ValueError('dy must have the shape of x and relu_bits one bit per element of it')
  coef = torch.empty((3, c), dtype=torch.float32, device=x.device)
  check(_lib.load().rigl_bn_bwd_reduce(m, c, _ptr(x), _ptr(relu_bits) if relu else None, _ptr(dy), _ptr(gamma), _ptr(saved[0]),
                                       _ptr(saved[1]), int(bool(relu)), _ptr(dgamma), _ptr(dbeta), _ptr(coef), _ptr(ws),
                                       ws.numel(), _stream()))
  return coef


# ----------------------------------------------------------------------------
# stateless random tensors (TensorFlow bit layout)
# ----------------------------------------------------------------------------
def stateless_random(n, seed0, seed1, dist, scale=1.0, shift=0.0, device=None,
                     out=None):
  """fp32 [n] = tf.random.stateless_{uniform|normal}([n], seed=[seed0, seed1])
  * scale + shift.  seed0 / seed1 are int32 (Python ints are wrapped)."""
  if dist not in ('uniform', 'normal'):
    raise ValueError('dist must be "uniform" or "normal"')
  if out is None:
    out = torch.empty(int(n), dtype=torch.float32, device=device)
  _req(out, torch.float32, 'out')
  check(_lib.load().rigl_stateless_random(_ptr(out), out.numel(), _i32(seed0), _i32(seed1),
                                          1 if dist == 'normal' else 0,
                                          float(scale), float(shift), _stream()))
  return out


def stateless_random_batched(items, device):
  """items: [(n, seed0, seed1, 'uniform'|'normal', scale, shift)] -> list of fp32 [n] tensors (views of one
  allocation, each starting on a 256-byte boundary), filled by ONE launch (rigl_stateless_random_batched)."""
  if not items:
    return []
  offs, total = [], 0
  for it in items:
    offs.append(total)
    total += (int(it[0]) + 63) // 64 * 64
  buf = torch.empty(max(total, 1), dtype=torch.float32, device=device)
  arr = (_lib.RandomItem * len(items))()
  outs = []
  for i, (n, s0, s1, dist, scale, shift) in enumerate(items):
    if dist not in ('uniform', 'normal'):
      raise ValueError('dist must be "uniform" or "normal"')
    t = buf[offs[i]:offs[i] + int(n)]
    outs.append(t)
    arr[i].out = t.data_ptr() if int(n) else None
    arr[i].n = int(n)
    arr[i].seed0, arr[i].seed1 = _i32(s0), _i32(s1)
    arr[i].dist = 1 if dist == 'normal' else 0
    arr[i].scale, arr[i].shift = float(scale), float(shift)
  check(_lib.load().rigl_stateless_random_batched(arr, len(items), _stream()))
  return outs


# ----------------------------------------------------------------------------
# dropout (keep mask from the stateless stream, step counter on the device)
# ----------------------------------------------------------------------------
_DROPOUT_DTYPES = {torch.bfloat16: 0, torch.float32: 1}


def _dropout_dtype(t, name):
  _req(t, getattr(t, 'dtype', None), name)
  if t.dtype not in _DROPOUT_DTYPES:
    raise TypeError('%s: expected bfloat16 or float32, got %s' % (name, t.dtype))
  return _DROPOUT_DTYPES[t.dtype]


def dropout_fwd(x, rate, seed0, step, y=None, bits=None):
  """(y, bits) = rigl_dropout_fwd: y = x / (1 - rate) where tf.random.stateless_uniform([n], seed=[seed0, step]) >= rate,
  else +0; ``bits`` uint8 [ceil(n / 8)], bit i % 8 of byte i / 8 = element i kept.  ``step``: DEVICE int32 [1], read by the
  kernel (``dropout_advance`` moves it on), so a replayed graph draws a fresh mask.  x: bf16 or fp32, any shape."""
  dt = _dropout_dtype(x, 'x')
  _req(step, torch.int32, 'step')
  if step.numel() != 1:
    raise ValueError('step must hold one int32')
  n = x.numel()
  if y is None:
    y = torch.empty_like(x)
  if bits is None:
    bits = torch.empty((n + 7) // 8, dtype=torch.uint8, device=x.device)
  _req(y, x.dtype, 'y')
  _req(bits, torch.uint8, 'bits')
  if y.numel() != n or bits.numel() < (n + 7) // 8:
    raise ValueError('y must have the shape of x and bits ceil(n / 8) bytes')
  check(_lib.load().rigl_dropout_fwd(_ptr(x), _ptr(y), _ptr(bits), n, dt, float(rate), _i32(seed0), _ptr(step), _stream()))
  return y, bits


def dropout_bwd(dy, bits, rate, dx=None):
  """dx = dy / (1 - rate) where the forward's stored ``bits`` say kept, else +0 (rigl_dropout_bwd)."""
  dt = _dropout_dtype(dy, 'dy')
  _req(bits, torch.uint8, 'bits')
  n = dy.numel()
  if dx is None:
    dx = torch.empty_like(dy)
  _req(dx, dy.dtype, 'dx')
  if dx.numel() != n or bits.numel() < (n + 7) // 8:
    raise ValueError('dx must have the shape of dy and bits ceil(n / 8) bytes')
  check(_lib.load().rigl_dropout_bwd(_ptr(dy), _ptr(bits), _ptr(dx), n, dt, float(rate), _stream()))
  return dx


def dropout_advance(step):
  """step += 1 on the device (rigl_dropout_advance), once per training forward."""
  _req(step, torch.int32, 'step')
  if step.numel() != 1:
    raise ValueError('step must hold one int32')
  check(_lib.load().rigl_dropout_advance(_ptr(step), _stream()))


# ----------------------------------------------------------------------------
# the CIFAR input pipeline (standardize, mirror pad, crop, flip, shuffle; step counter on the device)
# ----------------------------------------------------------------------------
def cifar_batch(images, labels, batch, step, out, out_labels, out_index=None, train=True, seed0=0, shard=0, n_shards=1):
  """rigl_cifar_batch: batch ``step`` of the dataset (``images`` uint8 [N, 32, 32, 3], ``labels`` int32 [N]) into ``out``
  ([batch, 32, 32, 3], bf16 or fp32), ``out_labels`` and, when given, ``out_index`` (int32 [batch], the dataset index of each
  image).  ``step``: DEVICE int32 [1], read by the kernel (``cifar_advance`` moves it on), so a replayed graph produces the
  next batch.  train: standardized, mirror-padded, randomly cropped and flipped images in the epoch's keyed order; eval:
  standardized images in dataset order, ``step`` the batch index, images past the end of the dataset left unwritten."""
  _req(images, torch.uint8, 'images')
  _req(labels, torch.int32, 'labels')
  _req(step, torch.int32, 'step')
  dt = _dropout_dtype(out, 'out')
  _req(out_labels, torch.int32, 'out_labels')
  _req(out_index, torch.int32, 'out_index', allow_none=True)
  if step.numel() != 1:
    raise ValueError('step must hold one int32')
  if images.dim() != 4 or tuple(images.shape[1:]) != (32, 32, 3):
    raise ValueError('images must be [N, 32, 32, 3] uint8 (HWC), got %s' % (tuple(images.shape),))
  n = images.shape[0]
  batch = int(batch)
  if labels.numel() != n:
    raise ValueError('labels must hold one int32 per image')
  if batch > 0 and (out.numel() != batch * 3072 or out_labels.numel() != batch or
                    (out_index is not None and out_index.numel() != batch)):
    raise ValueError('out must be [batch, 32, 32, 3] and out_labels / out_index [batch]')
  check(_lib.load().rigl_cifar_batch(_ptr(images), _ptr(labels), n, batch, 0 if train else 1, int(shard), int(n_shards),
                                     _i32(seed0), _ptr(step), _ptr(out), dt, _ptr(out_labels), _ptr(out_index), _stream()))


def cifar_advance(step):
  """step += 1 on the device (rigl_cifar_advance), once per batch."""
  _req(step, torch.int32, 'step')
  if step.numel() != 1:
    raise ValueError('step must hold one int32')
  check(_lib.load().rigl_cifar_advance(_ptr(step), _stream()))


# ----------------------------------------------------------------------------
# max pooling (glue)
# ----------------------------------------------------------------------------
def maxpool_fwd(d, x):
  """Returns (y, argmax) for the pooling geometry ``d`` (conv_desc with
  cin == cout); argmax is uint8, one byte per output element."""
  _req(x, torch.bfloat16, 'x')
  y = torch.empty((d.n, d.ho, d.wo, d.cout), dtype=torch.bfloat16, device=x.device)
  arg = torch.empty((d.n, d.ho, d.wo, d.cout), dtype=torch.uint8, device=x.device)
  check(_lib.load().rigl_maxpool_fwd(C.byref(d), _ptr(x), _ptr(y), _ptr(arg), _stream()))
  return y, arg


def maxpool_bwd(d, dy, arg):
  _req(dy, torch.bfloat16, 'dy')
  _req(arg, torch.uint8, 'argmax')
  dx = torch.empty((d.n, d.h, d.w, d.cin), dtype=torch.bfloat16, device=dy.device)
  check(_lib.load().rigl_maxpool_bwd(C.byref(d), _ptr(dy), _ptr(arg), _ptr(dx), _stream()))
  return dx


def bn_statistics(x, gamma, beta, running_mean, running_var, momentum, eps, partials=None):
  """The statistics half of bn_fwd (no apply pass): returns saved = fp32 [4, C] (mean, invstd, scale, shift) and updates
  the moving averages (rigl_bn_fwd_statistics)."""
  m, c, ws, parts = _bn_plan(x, partials)
  saved = torch.empty((4, c), dtype=torch.float32, device=x.device)
  check(_lib.load().rigl_bn_fwd_statistics(
      m, c, _ptr(x), _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var), float(momentum), float(eps),
      _ptr(saved[0]), _ptr(saved[1]), _ptr(saved[2]), _ptr(saved[3]), _ptr(partials), parts, _ptr(ws),
      ws.numel() if ws is not None else 0, _stream()))
  return saved


def bn_add_bn_fwd(x, x2, saved2, gamma, beta, running_mean, running_var, momentum, eps, relu, partials=None):
  """relu?(bn(x) + bn2(x2)) in one apply pass; ``saved2`` = bn_statistics(x2, ...).  Returns (y, saved, relu_bits|None)."""
  _req(x2, torch.bfloat16, 'x2')
  if x2.shape != x.shape:
    raise ValueError('x2 must have the shape of x')
  m, c, ws, parts = _bn_plan(x, partials)
  y = torch.empty_like(x)
  saved = torch.empty((4, c), dtype=torch.float32, device=x.device)
  bits = torch.empty(x.numel() // 8, dtype=torch.uint8, device=x.device) if relu else None
  check(_lib.load().rigl_bn_add_bn_fwd(
      m, c, _ptr(x), _ptr(x2), _ptr(saved2[2]), _ptr(saved2[3]), _ptr(gamma), _ptr(beta), _ptr(running_mean),
      _ptr(running_var), float(momentum), float(eps), int(bool(relu)), _ptr(y), _ptr(saved[0]), _ptr(saved[1]),
      _ptr(saved[2]), _ptr(saved[3]), _ptr(partials), parts, _ptr(bits),
      _ptr(ws), ws.numel() if ws is not None else 0, _stream()))
  return y, saved, bits


def bn_add_bn_bwd(x, x2, relu_bits, dy, gamma, saved, gamma2, saved2, dgamma, dbeta, dgamma2, dbeta2):
  """Gradients of relu(bn(x) + bn2(x2)) w.r.t. x and x2 (returns (dx, dx2)); the four parameter gradients are overwritten."""
  _req(x, torch.bfloat16, 'x')
  _req(x2, torch.bfloat16, 'x2')
  _req(dy, torch.bfloat16, 'dy')
  _req(relu_bits, torch.uint8, 'relu_bits')
  c = x.shape[-1]
  m = x.numel() // c
  lib = _lib.load()
  ws = workspace(lib.rigl_bn_add_bn_bwd_workspace_bytes(m, c), x.device)
  dx, dx2 = torch.empty_like(x), torch.empty_like(x2)
  check(lib.rigl_bn_add_bn_bwd(m, c, _ptr(x), _ptr(x2), _ptr(relu_bits), _ptr(dy), _ptr(gamma), _ptr(saved[0]), _ptr(saved[1]),
                               _ptr(gamma2), _ptr(saved2[0]), _ptr(saved2[1]), _ptr(dx), _ptr(dx2), _ptr(dgamma), _ptr(dbeta),
                               _ptr(dgamma2), _ptr(dbeta2), _ptr(ws), ws.numel(), _stream()))
  return dx, dx2


def bn_relu_maxpool_fwd(d, x, gamma, beta, running_mean, running_var, momentum, eps, partials=None):
  """maxpool(relu(batch_norm(x))) for the pooling geometry ``d`` without the activated tensor
  (rigl_bn_fwd_statistics + rigl_bn_relu_maxpool_fwd).  Returns (y, argmax, saved) -- saved = fp32 [4, C]
  (mean, invstd, scale, shift) as bn_fwd returns it."""
  saved = bn_statistics(x, gamma, beta, running_mean, running_var, momentum, eps, partials=partials)
  lib = _lib.load()
  y = torch.empty((d.n, d.ho, d.wo, d.cout), dtype=torch.bfloat16, device=x.device)
  arg = torch.empty((d.n, d.ho, d.wo, d.cout), dtype=torch.uint8, device=x.device)
  check(lib.rigl_bn_relu_maxpool_fwd(C.byref(d), _ptr(x), _ptr(saved[2]), _ptr(saved[3]), _ptr(y), _ptr(arg), _stream()))
  return y, arg, saved


def bn_relu_maxpool_bwd(d, x, dy, arg, gamma, saved, dgamma, dbeta):
  """Gradient of bn_relu_maxpool_fwd w.r.t. x; dgamma / dbeta (fp32 [C]) are overwritten."""
  _req(x, torch.bfloat16, 'x')
  _req(dy, torch.bfloat16, 'dy')
  _req(arg, torch.uint8, 'argmax')
  lib = _lib.load()
  ws = workspace(lib.rigl_bn_relu_maxpool_bwd_workspace_bytes(C.byref(d)), x.device)
  dx = torch.empty_like(x)
  check(lib.rigl_bn_relu_maxpool_bwd(C.byref(d), _ptr(x), _ptr(dy), _ptr(arg), _ptr(gamma), _ptr(saved[0]), _ptr(saved[1]),
                                     _ptr(saved[2]), _ptr(saved[3]), _ptr(dx), _ptr(dgamma), _ptr(dbeta), _ptr(ws),
                                     ws.numel(), _stream()))
  return dx


# ----------------------------------------------------------------------------
# classifier head glue
# ----------------------------------------------------------------------------
def global_avgpool_fwd(x):
  """[N, H, W, C] bf16 -> [N, C] bf16, fp32 accumulation."""
  _req(x, torch.bfloat16, 'x')
  n, h, w, c = x.shape
  y = torch.empty((n, c), dtype=torch.bfloat16, device=x.device)
  check(_lib.load().rigl_global_avgpool_fwd(n, h * w, c, _ptr(x), _ptr(y), _stream()))
  return y


def global_avgpool_bwd(dy, h, w):
  _req(dy, torch.bfloat16, 'dy')
  n, c = dy.shape
  dx = torch.empty((n, h, w, c), dtype=torch.bfloat16, device=dy.device)
  check(_lib.load().rigl_global_avgpool_bwd(n, h * w, c, _ptr(dy), _ptr(dx), _stream()))
  return dx


def global_avgpool_bwd_relu(dy, x):
  """dx = global_avgpool_bwd(dy) * [x > 0], x = the pooled [N, H, W, C] ReLU output (rigl_global_avgpool_bwd_relu)."""
  _req(dy, torch.bfloat16, 'dy')
  _req(x, torch.bfloat16, 'x')
  n, h, w, c = x.shape
  if tuple(dy.shape) != (n, c):
    raise ValueError('dy must be [N, C] of x')
  dx = torch.empty_like(x)
  check(_lib.load().rigl_global_avgpool_bwd_relu(n, h * w, c, _ptr(dy), _ptr(x), _ptr(dx), _stream()))
  return dx


def softmax_xent(logits, labels, label_smoothing=0.0, grad_scale=None, want_grad=True):
  """Per-row cross entropy (fp32 [rows]) of bf16 logits [rows, classes] against int64 labels with label
  smoothing, and the gradient of ``grad_scale * sum(rows)`` w.r.t. the logits (bf16; default scale 1/rows)."""
  _req(logits, torch.bfloat16, 'logits')
  _req(labels, torch.int64, 'labels')
  rows, k = logits.shape
  if labels.numel() != rows:
    raise ValueError('softmax_xent: %d labels for %d rows' % (labels.numel(), rows))
  loss = torch.empty(rows, dtype=torch.float32, device=logits.device)
  dz = torch.empty_like(logits) if want_grad else None
  check(_lib.load().rigl_softmax_xent(rows, k, _ptr(logits), _ptr(labels), float(label_smoothing),
                                      1.0 / rows if grad_scale is None else float(grad_scale), _ptr(loss), _ptr(dz),
                                      _stream()))
  return loss, dz


# ----------------------------------------------------------------------------
# evaluation: frozen-statistics batch norm and the eval metrics
# ----------------------------------------------------------------------------
def bn_infer_params(bns, out=None):
  """Scale / shift of the frozen batch norms ``bns`` (objects with gamma / beta variables, moving_mean, moving_variance,
  eps) in one launch (rigl_bn_infer_params_batched): returns fp32 [2, C] views of one buffer, in the order of ``bns``."""
  bns = list(bns)
  if not bns:
    return []
  total = sum(2 * b.moving_mean.numel() for b in bns)
  dev = bns[0].moving_mean.device
  if out is None:
    out = torch.empty(total, dtype=torch.float32, device=dev)
  _req(out, torch.float32, 'out')
  if out.numel() < total:
    raise ValueError('bn_infer_params: out holds %d floats < %d' % (out.numel(), total))
  arr = (_lib.BnInferItem * len(bns))()
  views, off = [], 0
  for i, b in enumerate(bns):
    c = b.moving_mean.numel()
    for t, nm in ((b.gamma.data, 'gamma'), (b.beta.data, 'beta'), (b.moving_mean, 'moving_mean'),
                  (b.moving_variance, 'moving_variance')):
      _req(t, torch.float32, nm)
      if t.numel() != c:
        raise ValueError('bn_infer_params: %s has %d channels, not %d' % (nm, t.numel(), c))
    v = out[off:off + 2 * c].view(2, c)
    arr[i] = _lib.BnInferItem(b.gamma.data.data_ptr(), b.beta.data.data_ptr(), b.moving_mean.data_ptr(),
                              b.moving_variance.data_ptr(), v.data_ptr(), c, float(b.eps))
    views.append(v)
    off += 2 * c
  check(_lib.load().rigl_bn_infer_params_batched(arr, len(bns), _stream()))
  return views


def _req_ss(ss, c, name='scale_shift'):
  _req(ss, torch.float32, name)
  if ss.dim() != 2 or ss.shape[0] not in (2, 4) or ss.shape[1] != c:
    raise ValueError('%s must be [2, %d] (or a [4, %d] saved block)' % (name, c, c))
  return ss[-2]


def bn_apply(x, scale_shift, relu=False, residual=None, y=None):
  """y = bf16(relu?(fmaf(x, scale, shift) (+ residual))) over the channel axis of x [..., C] (rigl_bn_apply): the training
  forward's apply pass with given scale / shift (``scale_shift`` fp32 [2, C], or a [4, C] saved block)."""
  _req(x, torch.bfloat16, 'x')
  _req(residual, torch.bfloat16, 'residual', allow_none=True)
  c = x.shape[-1]
  row = _req_ss(scale_shift, c)
  if residual is not None and residual.shape != x.shape:
    raise ValueError('residual must have the shape of x')
  if y is None:
    y = torch.empty_like(x)
  _req(y, torch.bfloat16, 'y')
  check(_lib.load().rigl_bn_apply(x.numel() // c, c, _ptr(x), _ptr(residual), _ptr(row), int(bool(relu)), _ptr(y), _stream()))
  return y


def bn_apply_pair(x, x2, scale_shift, scale_shift2, relu=True):
  """y = bf16(relu?(fmaf(x, scale, shift) + bf16(fmaf(x2, scale2, shift2)))) (rigl_bn_apply_pair): the projection block's
  tail with the rounding points of rigl_bn_add_bn_fwd."""
  _req(x, torch.bfloat16, 'x')
  _req(x2, torch.bfloat16, 'x2')
  if x2.shape != x.shape:
    raise ValueError('x2 must have the shape of x')
  c = x.shape[-1]
  r1, r2 = _req_ss(scale_shift, c), _req_ss(scale_shift2, c, 'scale_shift2')
  y = torch.empty_like(x)
  check(_lib.load().rigl_bn_apply_pair(x.numel() // c, c, _ptr(x), _ptr(x2), _ptr(r1), _ptr(r2), int(bool(relu)), _ptr(y),
                                       _stream()))
  return y


def bn_relu_maxpool_infer(d, x, scale_shift):
  """maxpool(bf16(relu(fmaf(x, scale, shift)))) for the pooling geometry ``d``, no argmax (rigl_bn_relu_maxpool_infer)."""
  _req(x, torch.bfloat16, 'x')
  row = _req_ss(scale_shift, d.cin)
  y = torch.empty((d.n, d.ho, d.wo, d.cout), dtype=torch.bfloat16, device=x.device)
  check(_lib.load().rigl_bn_relu_maxpool_infer(C.byref(d), _ptr(x), _ptr(row), _ptr(y), _stream()))
  return y


def eval_metrics(logits, labels, label_smoothing=0.0, topk=5, counts=None):
  """Per-row cross entropy (fp32 [rows], the bits of softmax_xent) and hit flags (int32 [rows]: top-1 | top-k << 1) of bf16
  logits [rows, classes] against int64 labels (rigl_eval_metrics); ``counts`` (int64 [3]: rows, top-1, top-k hits) is added to."""
  _req(logits, torch.bfloat16, 'logits')
  _req(labels, torch.int64, 'labels')
  _req(counts, torch.int64, 'counts', allow_none=True)
  if counts is not None and counts.numel() != 3:
    raise ValueError('counts must be int64 [3]')
  rows, k = logits.shape
  if labels.numel() != rows:
    raise ValueError('eval_metrics: %d labels for %d rows' % (labels.numel(), rows))
  loss = torch.empty(rows, dtype=torch.float32, device=logits.device)
  flags = torch.empty(rows, dtype=torch.int32, device=logits.device)
  check(_lib.load().rigl_eval_metrics(rows, k, _ptr(logits), _ptr(labels), float(label_smoothing), int(topk), _ptr(loss),
                                      _ptr(flags), _ptr(counts), _stream()))
  return loss, flags


# ----------------------------------------------------------------------------
# profiling
# ----------------------------------------------------------------------------
def tune_set(key, value):
  """Process-wide kernel-selection knob (rigl_tune_set).  The plan-dependent sizes cached on descriptors (_plan_cached)
  are keyed on the knob generation, so a descriptor made before the call asks the library again."""
  check(_lib.load().rigl_tune_set(key.encode(), int(value)))


def tune_unset(key):
  """Back to the knob's RIGL_<KEY> environment variable / built-in default (rigl_tune_unset)."""
  check(_lib.load().rigl_tune_unset(key.encode()))


def tune_get(key, default=-1):
  return int(_lib.load().rigl_tune_get(key.encode(), int(default)))


def mfma_peak_probe(device='cuda:0', blocks=2048, iters=2000, reps=5):
  """Dense bf16 MFMA rate of this box in TFLOP/s (register-only MFMA chains, best of ``reps``)."""
  lib = _lib.load()
  sink = torch.zeros(blocks * 256, dtype=torch.float32, device=device)
  best = 0.0
  for r in range(reps + 1):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    check(lib.rigl_probe_mfma_bf16(blocks, iters, _ptr(sink), _stream()))
    e.record()
    e.synchronize()
    if r:
      best = max(best, blocks * 4 * iters * 8 * 32768.0 / (s.elapsed_time(e) * 1e-3) / 1e12)
  return best


def prof_enable(on=True):
  check(_lib.load().rigl_prof_enable(int(bool(on))))


def prof_collect_launches(cap=1 << 16):
  """[(kind name, (h, w, cin, cout, k, stride), ms)] of every timed dispatch since the last collect, in launch order
  (rigl_prof_collect_launches; consumes the events like prof_collect)."""
  arr = (_lib.ProfLaunch * cap)()
  n = C.c_int64(0)
  check(_lib.load().rigl_prof_collect_launches(arr, cap, C.byref(n)))
  if n.value > cap:
    raise RuntimeError('prof_collect_launches: %d timed dispatches, room for %d (the rest were consumed and dropped): '
                       'collect more often or pass a larger cap' % (n.value, cap))
  return [(_lib.PROF_KINDS[arr[i].kind], tuple(arr[i].tag), float(arr[i].ms)) for i in range(min(n.value, cap))]


def prof_collect():
  """{kind: (milliseconds, launches)} accumulated since the last collect."""
  ms = (C.c_double * len(_lib.PROF_KINDS))()
  cnt = (C.c_int64 * len(_lib.PROF_KINDS))()
  check(_lib.load().rigl_prof_collect_kinds(ms, cnt, len(_lib.PROF_KINDS)))
  return {k: (ms[i], cnt[i]) for i, k in enumerate(_lib.PROF_KINDS)}
