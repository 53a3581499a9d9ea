"""The reference of the state snapshot kernels and the CPU path of rigl_amd.checkpoint -- no GPU.

  * tests/state_ref.py against Python big-integer sums on hand cases; every case has the property it is named for;
  * a NumPy model of the gather that walks a table the way the kernel does equals the reference on every case, and each of
    eight mutants of it is rejected by the case set;
  * TrainingState on a CPU graph: save / rebuild with other values / restore ends equal, a file saved twice is byte-identical,
    and every damaged or foreign file is refused with every tensor of the run unchanged.
"""
import json
import os
import struct

import numpy as np
import pytest

from tests import state_ref as R

torch = pytest.importorskip('torch')


# ---- the reference ---------------------------------------------------------------------------------------------------------
def test_digest_against_big_integers():
  assert R.digest(np.zeros(0, np.uint32)) == (0, 0)
  assert R.digest(np.array([5], np.uint32)) == (5, 5)
  assert R.digest(np.array([1, 2, 3], np.uint32)) == (6, 1 + 4 + 9)
  rng = np.random.RandomState(0)
  for n in (1, 2, 63, 64, 65, 1000):
    w = R.random_words(rng, n)
    assert R.digest(w) == R.digest_bigint(w)
  n = 100000
  w = np.full(n, 0xFFFFFFFF, np.uint32)
  exact = (2 ** 32 - 1) * n * (n + 1) // 2
  assert exact > 2 ** 64 and R.digest(w) == ((2 ** 32 - 1) * n, exact % 2 ** 64)


def test_offsets_and_image():
  offs, total = R.offsets([0, 4, 256, 260, 0, 8])
  assert offs == [0, 0, 256, 512, 1024, 1024] and total == 1280
  regs = [np.arange(1, 2, dtype=np.uint32), np.zeros(0, np.uint32), np.arange(65, dtype=np.uint32)]
  packed, dig = R.image(regs)
  assert packed.size == 256 + 0 + 512 and packed.dtype == np.uint8
  assert packed[:4].view(np.uint32)[0] == 1 and not packed[4:256].any()
  assert np.array_equal(packed[256:256 + 260].view(np.uint32), regs[2]) and not packed[516:].any()
  assert dig[1] == (0, 0) and dig[2] == R.digest_bigint(regs[2])


def test_the_constants_are_the_library_s():
  from rigl_amd import _lib
  assert (R.ALIGN, R.CHUNK, R.BATCH) == (_lib.STATE_ALIGN, _lib.STATE_CHUNK, _lib.STATE_BATCH)
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  txt = open(os.path.join(root, 'include', 'rigl_hip.h')).read()
  for name, v in (('RIGL_STATE_ALIGN', R.ALIGN), ('RIGL_STATE_CHUNK', R.CHUNK), ('RIGL_STATE_BATCH', R.BATCH)):
    assert '#define %s %d\n' % (name, v) in txt
  assert R.CHUNK % R.TILE == 0 and R.TILE % R.ROW == 0


def test_every_case_has_the_property_it_is_named_for():
  C = R.CASES
  for name in ('small', 'small_shifted'):
    assert C[name].words == [0, 1, 3, 4, 5, 63, 64, 65]
  assert set(C['small'].shift) == {0, 1, 2, 3} and 0 not in C['small_shifted'].shift
  for name in ('edges', 'edges_aligned'):
    for edge in (R.ROW, R.TILE, R.CHUNK, 2 * R.CHUNK):
      assert {edge - 1, edge, edge + 1} <= set(C[name].words)
  assert set(C['edges'].shift) == {0, 1, 2, 3} and set(C['edges_aligned'].shift) == {0}
  # every edge size is met at a shifted pointer and at an aligned one
  assert all(s != 0 or w in C['edges_aligned'].words for w, s in zip(C['edges'].words, C['edges'].shift))
  assert [len(C['table_%d' % n].words) for n in (1, 64, 65, 129)] == [1, 64, 65, 129]
  assert C['table_1_empty'].words == [0]
  for n in (64, 65, 129):
    w = C['table_%d' % n].words
    assert w[0] == 0 and w[-1] == 0 and w[63] == 0 and sum(1 for x in w if x == 0) == len({0, n - 1, 63})
    if n > 65:
      assert w[64] > 0                                    # the first region of the second launch holds data
  assert C['long'].words == [1048577] and -(-1048577 // R.CHUNK) > 3 * 8     # a grid of 3 gives a workgroup many chunks
  w = C['wrap'].regions()[0]
  assert w.size == 131072 and (w == 0xFFFFFFFF).all()
  tri = lambda n: (2 ** 32 - 1) * n * (n + 1) // 2
  assert tri(w.size) > 2 ** 64 and tri(R.WRAP_LEAST) >= 2 ** 64 > tri(R.WRAP_LEAST - 1)
  # the data: NaN payloads, -0.0 and subnormals are there
  r = np.concatenate(C['edges'].regions())
  f = r.view(np.float32)
  assert np.isnan(f).any() and (r == 0x80000000).any() and ((r & 0x7F800000 == 0) & (r & 0x007FFFFF != 0)).any()
  quiet = np.array([0x7FC00000, 0xFFC00000], np.uint32)
  assert (np.isnan(f) & ~np.isin(r, quiet)).any()          # a NaN with a payload


def test_carve_places_every_region_at_its_shift_between_guards():
  for case in R.CASES.values():
    if case.name in ('long', 'wrap'):
      continue
    regs = case.regions()
    buf, spans = case.carve(guard=64, regions=regs)
    prev_end = 0
    for (o, n), r, s in zip(spans, regs, case.shift):
      assert (o % 16) // 4 == s and o % 4 == 0 and n == 4 * r.size and o - prev_end >= 64
      assert np.array_equal(buf[o:o + n], r.view(np.uint8))
      prev_end = o + n
    assert buf.size - prev_end >= 64 and R.Case.outside_intact(buf, spans)


# ---- a model of the kernel's walk, and its mutants -----------------------------------------------------------------------
POISON = 0xFF
MUTANTS = ['pad_in_digest', 'pad_unwritten', 'i_not_i_plus_1', 's1_32_bit', 'align_128', 'tail_dropped', 'region_64_from_slot_0',
           'store_past']


def _model_digest(words, mutant):
  w = words.astype(np.uint64)
  first = 0 if mutant == 'i_not_i_plus_1' else 1
  with np.errstate(over='ignore'):
    s1 = int(w.sum(dtype=np.uint64))
    s2 = int((w * np.arange(first, first + w.size, dtype=np.uint64)).sum(dtype=np.uint64))
  return (s1 & 0xFFFFFFFF if mutant == 's1_32_bit' else s1), s2


def model_gather(case, mutant=None):
  """(packed image, digests): the table walked region by region out of the carved buffer into a poisoned image."""
  buf, spans = case.carve(guard=256, regions=case.regions())
  align = 128 if mutant == 'align_128' else R.ALIGN
  rnd = lambda n: -(-n // align) * align
  _, total = R.offsets([n for _, n in spans])
  packed = np.full(total + 2 * R.ALIGN, POISON, dtype=np.uint8)
  digests, off = [], 0
  for r, (o, n) in enumerate(spans):
    if mutant == 'region_64_from_slot_0' and r == R.BATCH:
      o, n = spans[0]
    src = buf[o:o + rnd(n)].copy().view(np.uint32)                # (with the guard's words behind the region)
    m = n // 4
    moved = m - m % 4 if mutant == 'tail_dropped' and o % 16 else m
    packed[off:off + 4 * moved] = src[:moved].view(np.uint8)
    if mutant != 'pad_unwritten':
      packed[off + 4 * moved:off + rnd(n)] = 0 if moved == m else POISON
      packed[off + n:off + rnd(n)] = 0
    if mutant == 'store_past':
      packed[off + n:off + n + 4] = src[m:m + 1].view(np.uint8) if src.size > m else POISON
    digests.append(_model_digest(src if mutant == 'pad_in_digest' else src[:moved], mutant))
    off += rnd(spans[r][1])
  return packed[:total], digests


def model_scatter(case, mutant=None):
  """(the carved destination buffer, spans, digests) after scattering the reference image into sentinel-filled regions."""
  regs = case.regions()
  packed, _ = R.image(regs)
  buf, spans = case.carve(guard=256)
  offs, _ = R.offsets([n for _, n in spans])
  digests = []
  for (o, n), off in zip(spans, offs):
    extra = 4 if mutant == 'store_past' else 0
    src = np.concatenate([packed, np.zeros(4, np.uint8)])[off:off + n + extra]
    buf[o:o + n + extra] = src
    digests.append(R.digest(src[:n].copy()))
  return buf, spans, digests


def _same(case, out):
  packed, digests = R.image(case.regions())
  return np.array_equal(out[0], packed) and out[1] == digests


def test_the_model_is_the_reference_on_every_case():
  for case in R.CASES.values():
    assert _same(case, model_gather(case)), case.name
    regs = case.regions()
    buf, spans, digests = model_scatter(case)
    assert R.Case.outside_intact(buf, spans) and digests == [R.digest(r) for r in regs], case.name
    assert all(np.array_equal(buf[o:o + n], r.view(np.uint8)) for (o, n), r in zip(spans, regs)), case.name


@pytest.mark.parametrize('mutant', MUTANTS)
def test_every_mutant_is_rejected_by_the_case_set(mutant):
  caught = []
  for case in R.CASES.values():
    if not _same(case, model_gather(case, mutant)):
      caught.append(case.name)
    elif mutant == 'store_past':
      buf, spans, _ = model_scatter(case, mutant)
      if not R.Case.outside_intact(buf, spans):
        caught.append(case.name)
  assert caught, 'no case tells the mutant %s from the reference' % mutant
  print('mutant %-24s caught by %s' % (mutant, caught))


# ---- the CPU path of TrainingState ---------------------------------------------------------------------------------------
def _run(seed, optimizer='momentum', names=('a', 'b', 'c'), shape_b=(5, 7), fill=True):
  """A CPU graph with three variables (two masked kernels and a bias), arenas and slots filled by hand from ``seed``."""
  from rigl_amd import checkpoint, train, variables as V
  g = V.Graph('cpu')
  la = g.add_masked_layer(names[0], (3, 3, 4, 6), True)
  lb = g.add_masked_layer(names[1], shape_b, True)
  g.add_variable(names[2] + '/biases', (6,), V.KIND_OTHER)
  gs = g.get_or_create_global_step()
  if optimizer == 'adam':
    inner = train.AdamOptimizer(0.001, graph=g)
  else:
    inner = train.MomentumOptimizer(0.1, 0.9, use_nesterov=True, graph=g)
  state = checkpoint.TrainingState(g, inner, extra={'seed': seed, 'note': 'cpu'})
  if fill:
    rng = np.random.RandomState(seed)
    g.W.copy_(torch.from_numpy(R.random_words(rng, g.W.numel()).view(np.float32).copy()))
    g.BITS.copy_(torch.from_numpy(rng.randint(0, 1 << 32, size=g.BITS.numel(), dtype=np.uint64).astype(np.uint32).view(np.int32).copy()))
    inner._slot.copy_(torch.from_numpy(R.random_words(rng, g.W.numel()).view(np.float32).copy()))
    if optimizer == 'adam':
      inner._slot_v.copy_(torch.from_numpy(rng.rand(g.W.numel()).astype(np.float32)))
      inner._beta_powers.copy_(torch.tensor([0.9 ** seed, 0.999 ** seed]))
    gs.value = 100 + seed
  return g, inner, state, (la, lb)


def _bits_of(g, inner):
  out = [g.W.numpy().view(np.uint32).copy(), g.BITS.numpy().copy(), inner._slot.numpy().view(np.uint32).copy()]
  if getattr(inner, '_slot_v', None) is not None:
    out += [inner._slot_v.numpy().view(np.uint32).copy(), inner._beta_powers.numpy().view(np.uint32).copy()]
  return out


def _equal(a, b):
  return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_cpu_save_rebuild_restore(tmp_path):
  from rigl_amd import checkpoint
  path = str(tmp_path / 'ckpt')
  g, inner, state, layers = _run(1)
  assert state.region_names() == ['graph/W', 'graph/BITS', 'slot/momentum']
  want = _bits_of(g, inner)
  mask_a = layers[0].mask.bits.numpy().copy()
  state.save(path)
  assert not os.path.exists(path + '.tmp')
  first = open(path, 'rb').read()
  state.save(path)
  assert open(path, 'rb').read() == first                     # a file saved twice is byte-identical
  assert first[:8] == checkpoint.MAGIC and len(first) % 256 == 0
  hlen = struct.unpack('<Q', first[8:16])[0]
  header = json.loads(first[16:16 + hlen].decode('utf-8'))
  assert [r[0] for r in header['regions']] == state.region_names() and header['scalars']['global_step'] == 101
  assert header['regions'][0][2:] == list(R.digest(want[0]))   # the file's digests are the reference's
  packed, _ = R.image([want[0], want[1].view(np.uint32), want[2]])
  assert first[-packed.size:] == packed.tobytes()             # ... and its image the reference's
  g2, inner2, state2, layers2 = _run(2)
  assert not _equal(_bits_of(g2, inner2), want)
  w_tensor, view_a = g2.W, layers2[0].weights.data
  assert state2.restore(path) == {'seed': 1, 'note': 'cpu'}
  assert _equal(_bits_of(g2, inner2), want) and int(g2.global_step.value) == 101
  assert g2.W is w_tensor and layers2[0].weights.data is view_a and g2.shadows_dirty      # in place: nothing was rebound
  np.testing.assert_array_equal(layers2[0].mask.bits.numpy(), mask_a)
  # from a Snapshot, with no file in between
  g3, inner3, state3, _ = _run(3)
  state3.restore(state.snapshot())
  assert _equal(_bits_of(g3, inner3), want)


def test_cpu_adam_and_wrapper_scalars(tmp_path):
  from rigl_amd import checkpoint, sparse_optimizers as SO
  path = str(tmp_path / 'ckpt')
  g, inner, _, _ = _run(4, 'adam')
  opt = SO.SparseRigLOptimizer(inner, 0, 1000, 5)
  opt._last_update_step = 95
  state = checkpoint.TrainingState(g, opt)
  assert state.region_names() == ['graph/W', 'graph/BITS', 'slot/m', 'slot/v', 'adam/beta_powers']
  want = _bits_of(g, inner)
  state.save(path)
  g2, inner2, _, _ = _run(5, 'adam')
  opt2 = SO.SparseRigLOptimizer(inner2, 0, 1000, 5)
  checkpoint.TrainingState(g2, opt2).restore(path)
  assert _equal(_bits_of(g2, inner2), want) and opt2._last_update_step == 95 and int(g2.global_step.value) == 104
  # the same arenas under the bare inner optimizer are another run: the wrapper's class is part of the fingerprint
  g3, inner3, state3, _ = _run(6, 'adam')
  with pytest.raises(checkpoint.CheckpointError, match='wrapper'):
    state3.restore(path)


def _damaged(first):
  """(what, bytes) of every damaged file: truncations and one flipped byte in the header, its padding and a region (a byte of
  the padding between two regions: in the test)."""
  hlen = struct.unpack('<Q', first[8:16])[0]
  data0 = -(-(16 + hlen) // 256) * 256
  assert data0 > 16 + hlen                                     # there is header padding to flip
  flip = lambda at: first[:at] + bytes([first[at] ^ 0x10]) + first[at + 1:]
  out = [('truncated by a byte', first[:-1]), ('truncated to the header', first[:data0]), ('truncated inside the header', first[:40]),
         ('a byte appended', first + b'\0'), ('magic', flip(3)), ('header length', flip(9))]
  out += [('header byte %d' % at, flip(at)) for at in (16, 16 + hlen // 2, 16 + hlen - 1)]
  digit = first.index(b'"global_step":') + len(b'"global_step":')
  out.append(('a digit of the global step', first[:digit] + (b'2' if first[digit:digit + 1] != b'2' else b'3') + first[digit + 1:]))
  out.append(('header padding', flip(data0 - 1)))
  out.append(('region byte', flip(data0 + 100)))
  return out


def test_cpu_refusals_leave_the_run_unchanged(tmp_path):
  from rigl_amd import checkpoint
  path = str(tmp_path / 'ckpt')
  g, inner, state, _ = _run(1)
  state.save(path)
  first = open(path, 'rb').read()
  g2, inner2, state2, _ = _run(2)
  before = _bits_of(g2, inner2)
  bad = str(tmp_path / 'bad')
  cases = _damaged(first)
  assert len(cases) >= 12
  for what, raw in cases:
    assert raw != first, what
    with open(bad, 'wb') as f:
      f.write(raw)
    with pytest.raises(checkpoint.CheckpointError):
      state2.restore(bad)
    assert _equal(_bits_of(g2, inner2), before) and int(g2.global_step.value) == 102, what
  # a padding byte between two regions (BITS is shorter than 256 bytes)
  offs, _ = R.offsets(state._sizes)
  hlen = struct.unpack('<Q', first[8:16])[0]
  data0 = -(-(16 + hlen) // 256) * 256
  assert state._sizes[1] % 256 != 0
  at = data0 + offs[1] + state._sizes[1] + 1
  with open(bad, 'wb') as f:
    f.write(first[:at] + b'\x01' + first[at + 1:])
  with pytest.raises(checkpoint.CheckpointError, match='padding'):
    state2.restore(bad)
  assert _equal(_bits_of(g2, inner2), before)
  # foreign files: a variable renamed, a shape changed, Adam into momentum
  for kw, match in ((dict(names=('a', 'b2', 'c')), 'b2'), (dict(shape_b=(7, 5)), 'variables'), (dict(optimizer='adam'), 'optimizer')):
    g3, inner3, state3, _ = _run(3, **kw)
    state3.save(bad)
    with pytest.raises(checkpoint.CheckpointError, match=match):
      state2.restore(bad)
    assert _equal(_bits_of(g2, inner2), before) and int(g2.global_step.value) == 102, kw
  state2.restore(path)                                         # and the good file still goes in
  assert _equal(_bits_of(g2, inner2), _bits_of(g, inner))


# ---- a save on a writer thread against the next snapshot -----------------------------------------------------------------
class _AskedLock:
  """A Snapshot's lock that tells when a thread other than ``owner`` asks for it."""

  def __init__(self, lock, owner_box, asked):
    self._lock, self._owner_box, self._asked = lock, owner_box, asked

  def __enter__(self):
    import threading
    if threading.current_thread() is not self._owner_box[0]:
      self._asked.set()
    self._lock.acquire()
    return self

  def __exit__(self, *exc):
    self._lock.release()


class _SlowFile:
  """A binary file object that, behind the first block of the image, holds its writer until the training thread has asked for
  the snapshot's lock (or, where nothing ever asks, for ``patience`` seconds: only a broken implementation waits them out)."""

  def __init__(self, started, asked, patience=5.0):
    import io
    self.buf, self.calls, self.started, self.asked, self.patience = io.BytesIO(), 0, started, asked, patience

  def write(self, data):
    self.calls += 1
    self.buf.write(data)
    if self.calls == 2:                                          # the head, then the first block of the image
      self.started.set()
      self.asked.wait(self.patience)


def _set_all(g, inner, seed):
  rng = np.random.RandomState(seed)
  g.W.copy_(torch.from_numpy(rng.rand(g.W.numel()).astype(np.float32)))
  inner._slot.copy_(torch.from_numpy(rng.rand(g.W.numel()).astype(np.float32)))


def test_a_save_in_flight_is_not_torn_by_the_next_snapshot(monkeypatch):
  import threading
  from rigl_amd import checkpoint
  monkeypatch.setattr(checkpoint, 'WRITE_BLOCK', 256)           # the image goes out in many blocks
  g, inner, state, _ = _run(1)
  snap1 = state.snapshot()
  assert snap1._shared and snap1._packed is state._host          # the image lives in the ONE shared host buffer
  expected = snap1.tobytes()
  assert len(expected) > 4 * 256
  started, asked, owner = threading.Event(), threading.Event(), [None]
  snap1._lock = _AskedLock(snap1._lock, owner, asked)
  slow = _SlowFile(started, asked)
  writer = threading.Thread(target=snap1.write, args=(slow,))
  owner[0] = writer
  writer.start()
  assert started.wait(10.0)                                      # the writer is inside the image
  _set_all(g, inner, 99)                                         # training goes on ...
  snap2 = state.snapshot()                                       # ... and takes the next snapshot: it must wait for the writer
  writer.join(10.0)
  assert not writer.is_alive() and asked.is_set()
  assert slow.buf.getvalue() == expected                         # not a byte of the second image in the first file
  assert snap2.tobytes() != expected and snap2._packed is state._host
  assert not snap1._shared and snap1._packed is not state._host and snap1.tobytes() == expected   # it moved out, intact
  # what the first file holds restores the first state
  g2, inner2, state2, _ = _run(2)
  state2.restore(snap1)
  assert _equal(_bits_of(g2, inner2)[:1], [np.frombuffer(expected[-state._packed_bytes:][:g.W.numel() * 4], np.uint32)])


def test_a_saved_or_dropped_snapshot_costs_the_next_one_no_copy(tmp_path):
  from rigl_amd import checkpoint
  g, inner, state, _ = _run(1)
  snap = state.snapshot()
  snap.save(str(tmp_path / 'a'))                                 # keep=False: the image is on disk and let go of
  assert snap._packed is None and not snap._shared
  with pytest.raises(RuntimeError, match='released'):
    state.restore(snap)
  with pytest.raises(RuntimeError, match='released'):
    snap.tobytes()
  copies = []
  real = checkpoint.Snapshot._own
  def counted(self):
    before = self._packed
    real(self)
    copies.append(self._packed is not before)
  checkpoint.Snapshot._own = counted
  try:
    s2 = state.snapshot()                                        # the one before was saved: nothing to move
    assert copies in ([], [False])
    del s2
    import gc
    gc.collect()
    s3 = state.snapshot()                                        # the one before was dropped: nothing to move
    assert not any(copies)
    s3.save(str(tmp_path / 'b'), keep=True)                      # kept for a rollback: the next snapshot moves it out
    _set_all(g, inner, 5)
    s4 = state.snapshot()
    assert copies[-1] is True and s3._packed is not state._host and s4._packed is state._host
    state.restore(s3)                                            # ... and it still restores what it held
    assert open(str(tmp_path / 'b'), 'rb').read() == s3.tobytes() == state.snapshot().tobytes()
  finally:
    checkpoint.Snapshot._own = real
