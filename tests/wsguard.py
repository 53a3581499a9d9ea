"""A guarded, exactly-sized, poisoned stand-in for ``rigl_amd.ops.workspace`` -- TEST INFRASTRUCTURE, never imported by the
product.

The product's pool (ops.workspace) never hands out less than 1 MiB, grows by 1.5x, reuses one buffer per device and user,
and the wrappers pass ``ws.numel()`` as workspace_bytes: a ``*_workspace_bytes`` query that under-reports, a kernel that
reads scratch it did not initialise, and a missing size check are all invisible behind it.  Here every request is carved
fresh out of a sentinel-filled uint8 arena as

    [ guard (1 MiB) | payload (exactly nbytes, on a 256-byte boundary, filled with the poison) | guard (1 MiB) ]

so that ``ws.numel() == nbytes`` reaches the C ABI, a contiguous overrun of up to 1 MiB lands in the test's own allocation
(it cannot fault the device) and is reported, and state left by "the previous kernel" is 0x00 or 0xFF bytes (as fp32 0xFF
is a NaN, as a counter -1 / 2^32 - 1) instead of a plausible value.

  g = GuardedWorkspace(poison=0xFF)
  with installed(g):                 # swaps the attribute on the rigl_amd.ops module, restores it on exit
    ops.conv_wgrad(...)              # every ops.workspace(nbytes, device, tag) call is now g(nbytes, device, tag)
    g.check('wgrad')                 # synchronises; every guard of every region handed out must still be the sentinel

``check`` names the tag, the size and the offset of the first changed byte (relative to the payload's start: negative in
front, >= nbytes behind), records per request the high-water mark -- one past the last payload byte that differs from the
poison; reported, never asserted: a kernel may legitimately write bytes equal to the poison -- and then takes the regions
back (their payload bytes become sentinel again), so a long walk needs no more memory than its largest step.
Not for graph capture (a captured graph holds addresses): train.GraphedStep stays on the pool.
"""
import contextlib

import torch

GUARD = 1 << 20                            # bytes of guard on each side of a payload
ALIGN = 256                                # the unit every layout in csrc/ aligns to; what include/rigl_hip.h asks of a caller
SENTINEL = 0xA5                            # guard bytes: neither poison
POISONS = (0x00, 0xFF)
_BLOCK = 4096                              # granularity of the first level of the high-water search


def _align(n):
  return -(-int(n) // ALIGN) * ALIGN


class GuardedWorkspace:
  """Callable with the signature of ops.workspace.  ``requests``, ``max_bytes``, ``max_used`` and ``log`` (one (tag, nbytes,
  used) per checked request) accumulate over the object's life; ``live`` are the regions handed out since the last check."""

  def __init__(self, poison=0xFF, guard=GUARD, arena_bytes=64 << 20):
    assert 0 <= poison <= 0xFF and poison != SENTINEL
    assert guard % ALIGN == 0 and guard > 0
    self.poison, self.guard, self.arena_bytes = int(poison), int(guard), int(arena_bytes)
    self.arenas = {}                       # device -> list of [buffer, first aligned offset, bump pointer]
    self.live = []                         # (buffer, payload offset, nbytes, tag)
    self.requests = self.max_bytes = self.max_used = 0
    self.log = []

  # -- ops.workspace(nbytes, device, tag) -------------------------------------------------------------------------------
  def __call__(self, nbytes, device, tag=''):
    nbytes = int(nbytes)
    assert nbytes >= 0, 'workspace request of %d bytes' % nbytes
    device = torch.device(device)
    span = self.guard + _align(nbytes) + self.guard
    chain = self.arenas.setdefault(device, [])
    for a in chain:
      if a[2] + span <= a[0].numel():
        break
    else:
      buf = torch.full((max(self.arena_bytes, span) + ALIGN,), SENTINEL, dtype=torch.uint8, device=device)
      first = (-buf.data_ptr()) % ALIGN    # (the allocators align further than this; a CPU tensor need not)
      a = [buf, first, first]
      chain.append(a)
    buf, off = a[0], a[2] + self.guard
    a[2] += span
    ws = buf[off:off + nbytes]
    if nbytes:
      ws.fill_(self.poison)
      assert ws.data_ptr() % ALIGN == 0
    assert ws.numel() == nbytes and ws.is_contiguous()
    self.live.append((buf, off, nbytes, tag))
    self.requests += 1
    self.max_bytes = max(self.max_bytes, nbytes)
    return ws

  # -- the checks -------------------------------------------------------------------------------------------------------
  def _high_water(self, payload):
    """One past the last byte of ``payload`` that differs from the poison (0: untouched, or only poison-valued writes)."""
    n = payload.numel()
    if n == 0:
      return 0
    ne = payload != self.poison
    whole = n // _BLOCK * _BLOCK
    tail = ne[whole:]
    if tail.numel() and bool(tail.any()):
      return whole + int(tail.nonzero()[-1]) + 1
    if whole == 0:
      return 0
    blocks = ne[:whole].view(-1, _BLOCK)
    hit = blocks.any(dim=1).nonzero()
    if hit.numel() == 0:
      return 0
    b = int(hit[-1])
    return b * _BLOCK + int(blocks[b].nonzero()[-1]) + 1

  def check(self, where=''):
    """Synchronises, asserts that every guard of every region handed out since the last check is byte-identical to the
    sentinel, records the high-water marks and takes the regions back.  Returns the [(tag, nbytes, used)] of this check."""
    if any(d.type == 'cuda' for d in self.arenas):
      torch.cuda.synchronize()
    out = []
    try:
      flags = [torch.stack(((buf[off - self.guard:off] != SENTINEL).any(),
                            (buf[off + nbytes:off + _align(nbytes) + self.guard] != SENTINEL).any()))
               for buf, off, nbytes, _ in self.live]
      touched = torch.stack(flags).cpu().tolist() if flags else []     # (one transfer for all regions)
      for (buf, off, nbytes, tag), (front, back) in zip(self.live, touched):
        for hit, side, lo, hi in ((front, 'in front of', off - self.guard, off),
                                  (back, 'behind', off + nbytes, off + _align(nbytes) + self.guard)):
          if hit:
            ne = (buf[lo:hi] != SENTINEL).nonzero()
            pos = int(ne[0]) + lo - off
            raise AssertionError(
                '%sworkspace "%s" of %d bytes: wrote %s the payload: %d guard bytes changed, the first at offset %d '
                '(the payload is [0, %d))' % (where and where + ': ', tag, nbytes, side, int(ne.numel()), pos, nbytes))
        used = self._high_water(buf[off:off + nbytes])
        self.max_used = max(self.max_used, used)
        out.append((tag, nbytes, used))
      self.log.extend(out)
    finally:
      self._recycle()
    return out

  def _recycle(self):
    for buf, off, nbytes, _ in self.live:
      if nbytes:
        buf[off:off + nbytes].fill_(SENTINEL)
    self.live = []
    for chain in self.arenas.values():
      for a in chain:
        a[2] = a[1]

  def summary(self):
    return {'requests': self.requests, 'max_bytes': self.max_bytes, 'max_used': self.max_used}


@contextlib.contextmanager
def installed(guard, ops=None):
  """``rigl_amd.ops.workspace`` is ``guard`` inside the block and what it was before on exit, whatever happens inside."""
  if ops is None:
    from rigl_amd import ops
  before = ops.workspace
  ops.workspace = guard
  try:
    yield guard
  finally:
    ops.workspace = before
