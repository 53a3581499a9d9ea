"""tests/wsguard.py checked without a GPU, on CPU tensors: what a request looks like (exact length, 256-byte boundary, poison
fill, 1 MiB of sentinel on both sides), that ``installed`` swaps and restores ``rigl_amd.ops.workspace``, and the guard SEEN
FAILING -- a stand-in "kernel" that stays inside its payload passes, one that stores a single byte behind it or in front of
it is rejected with the tag, the size and the offset in the message.  (The overrun mutants run here only, never on a GPU.)"""
import pytest
import torch

from rigl_amd import ops
from tests import wsguard as G


def _around(ws, lo, hi):
  """The bytes [lo, hi) relative to the payload's start, read from the arena the payload was carved from."""
  base = ws._base if ws._base is not None else ws
  off = ws.storage_offset() if ws.numel() else None
  assert off is not None
  return base[off + lo:off + hi]


@pytest.mark.parametrize('poison', G.POISONS)
@pytest.mark.parametrize('nbytes', [1, 255, 256, 257, 4096, 70001, (1 << 20) + 3])
def test_request_is_exact_aligned_poisoned_and_guarded(poison, nbytes):
  g = G.GuardedWorkspace(poison=poison)
  ws = g(nbytes, 'cpu', 'probe')
  assert ws.dtype == torch.uint8 and ws.is_contiguous()
  assert ws.numel() == nbytes                                  # what the wrappers pass as workspace_bytes
  assert ws.data_ptr() % 256 == 0
  assert bool((ws == poison).all())
  assert bool((_around(ws, -G.GUARD, 0) == G.SENTINEL).all())
  assert bool((_around(ws, nbytes, nbytes + G.GUARD) == G.SENTINEL).all())
  assert g.check() == [('probe', nbytes, 0)]
  assert g.summary() == {'requests': 1, 'max_bytes': nbytes, 'max_used': 0}


def test_poisons_cover_zero_and_all_ones():
  assert 0x00 in G.POISONS and 0xFF in G.POISONS and G.SENTINEL not in G.POISONS
  ws = G.GuardedWorkspace(poison=0xFF)(16, 'cpu')
  assert bool(torch.isnan(ws.view(torch.float32)).all())       # as fp32 a NaN,
  assert ws.view(torch.int32).tolist() == [-1] * 4             # as a counter -1


def test_zero_bytes_is_a_zero_length_view_between_two_guards():
  g = G.GuardedWorkspace()
  a = g(0, 'cpu', 'empty')
  b = g(64, 'cpu', 'next')
  assert a.numel() == 0 and a.dtype == torch.uint8
  # the next region starts two whole guards further on: nothing of the empty one overlaps it
  assert b.storage_offset() - a.storage_offset() == 2 * G.GUARD
  assert [r[:2] for r in g.check()] == [('empty', 0), ('next', 64)]


def test_regions_of_one_check_are_disjoint_and_fresh():
  g = G.GuardedWorkspace(poison=0x00)
  a = g(1000, 'cpu', 'a')
  a.fill_(7)
  b = g(1000, 'cpu', 'b')                                      # the pool would have handed out a's bytes again
  assert bool((b == 0).all()) and bool((a == 7).all())
  assert abs(b.storage_offset() - a.storage_offset()) >= 1000 + 2 * G.GUARD - 256
  g.check()
  c = g(1000, 'cpu', 'c')                                      # after a check the bytes are reused -- poisoned again
  assert bool((c == 0).all())
  g.check()


def test_a_request_larger_than_the_arena_gets_its_own():
  g = G.GuardedWorkspace(arena_bytes=4 << 20)
  small = g(100, 'cpu', 'small')
  big = g(6 << 20, 'cpu', 'big')
  assert big.numel() == 6 << 20 and big.data_ptr() % 256 == 0
  big[-1] = 1
  small[0] = 1
  assert g.check() == [('small', 100, 1), ('big', 6 << 20, 6 << 20)]


def test_writes_inside_the_payload_pass_and_set_the_high_water_mark():
  g = G.GuardedWorkspace(poison=0xFF)
  ws = g(70001, 'cpu', 'inside')
  ws[:5000] = 3                                                # the stand-in kernel: first and last byte included
  ws[70000] = 9
  assert g.check('inside') == [('inside', 70001, 70001)]
  ws = g(70001, 'cpu', 'partly')
  ws[:12345] = 3
  ws[20000:20010] = 0xFF                                       # a write equal to the poison is invisible: reported, never asserted
  assert g.check() == [('partly', 70001, 12345)]
  assert g.summary() == {'requests': 2, 'max_bytes': 70001, 'max_used': 70001}


@pytest.mark.parametrize('nbytes', [1024, 1000, 0])
def test_one_byte_behind_the_payload_is_caught(nbytes):
  g = G.GuardedWorkspace()
  before = g(64, 'cpu', 'bystander')
  ws = g(nbytes, 'cpu', 'slabs')
  _around(before, 0, 64).fill_(1)
  base = ws._base
  base[ws.storage_offset() + nbytes] = 0                       # the mutant: a store one byte past the declared size
  with pytest.raises(AssertionError) as e:
    g.check('wgrad')
  msg = str(e.value)
  assert 'wgrad' in msg and '"slabs"' in msg and '%d bytes' % nbytes in msg and 'behind' in msg
  assert 'first at offset %d ' % nbytes in msg
  assert g.live == []                                          # the regions were taken back all the same
  ok = g(nbytes, 'cpu', 'again')
  assert g.check() == [('again', nbytes, 0)]                   # ... and the arena is whole again
  del ok


def test_one_byte_in_front_of_the_payload_is_caught():
  g = G.GuardedWorkspace()
  ws = g(4096, 'cpu', 'state')
  ws._base[ws.storage_offset() - 1] = 0                        # the mutant: index -1
  with pytest.raises(AssertionError) as e:
    g.check()
  assert '"state"' in str(e.value) and 'in front of' in str(e.value) and 'first at offset -1 ' in str(e.value)


def test_a_far_overrun_inside_the_guard_is_caught():
  g = G.GuardedWorkspace()
  ws = g(512, 'cpu', 'far')
  ws._base[ws.storage_offset() + 512 + G.GUARD - 1] = 0        # the last byte of the guard: one slab further on
  with pytest.raises(AssertionError):
    g.check()


def test_installed_swaps_ops_workspace_and_restores_it():
  pool = ops.workspace
  g = G.GuardedWorkspace()
  with G.installed(g) as inside:
    assert inside is g and ops.workspace is g
    ws = ops.workspace(300, 'cpu', 'tag')                      # the call the wrappers make
    assert ws.numel() == 300
    g.check()
  assert ops.workspace is pool
  with pytest.raises(RuntimeError):
    with G.installed(g):
      raise RuntimeError('a failing test body')
  assert ops.workspace is pool
  assert g.requests == 1
