"""The row-streaming dgrad with a masked addend (rowstream.hpp MODE 3, rigl_masked_conv2d_bwd_masked): the 256 <- 64 dgrad of a
bottleneck block's first conv receives the shortcut's gradient UNMASKED together with the 1-bit ReLU mask k_fwd_apply left and
computes bf16(bf16(acc) + (bit ? addend : 0)).

Expected: dX (and dW) bit-equal to the same call given the addend already masked (what rigl_bn_bwd's dresidual holds: the
gradient where the bit is set, +0 elsewhere).  Shapes: M = 2 x 47 x 47 = 4 418 rows with knob "rowstream" = 2 (every legal layer;
ragged: the last row fragment is partial and waves own no fragment) and M = 8 x 56 x 56 = 25 088 rows by default.  Bits are
random with one all-off and one all-on row.  dX is carved from a sentinel-filled buffer (tests/exactref.py guarded) and the
guard bands on both sides must be intact.
"""
import pytest

torch = pytest.importorskip('torch')

from tests import bn_ref as R  # noqa: E402
from tests import exactref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CIN, COUT = 256, 64          # the conv is 256 -> 64; its dgrad is the 256 <- 64 GEMM


@pytest.mark.parametrize('shape,knob', (((2, 47, 47), 2), ((8, 56, 56), None)), ids=('2x47x47-rowstream2', '8x56x56-default'))
def test_masked_addend_equals_premasked_addend(shape, knob):
  from rigl_amd import ops
  n, h, w = shape
  m = n * h * w
  if knob is not None:
    ops.tune_set('rowstream', knob)
  try:
    d = ops.conv_desc(n, h, w, CIN, COUT, 1, 1, 1, 0, 0, h, w)
    gen = torch.Generator(device='cpu').manual_seed(3 + m)
    x = (torch.randn(n, h, w, CIN, generator=gen) * 0.5).to(torch.bfloat16).to(DEV)
    dy = (torch.randn(n, h, w, COUT, generator=gen) * 0.5).to(torch.bfloat16).to(DEV)
    addend = torch.randn(n, h, w, CIN, generator=gen).to(torch.bfloat16).to(DEV)
    wf = (torch.randn(CIN * COUT, generator=gen) * 0.1).to(DEV)
    hwio = torch.empty(CIN * COUT, dtype=torch.bfloat16, device=DEV)
    ops.pack_weights(wf, None, CIN, COUT, hwio, None)
    on = torch.rand(m, CIN, generator=gen) < 0.5
    on[0] = False
    on[1] = True
    on[m - 1, 1::2] = True
    bits = R.pack_bits(on).to(DEV)
    masked = torch.where(on.to(DEV).reshape(n, h, w, CIN), addend, torch.zeros_like(addend))
    dw0 = torch.full((CIN * COUT,), 7.0, device=DEV)
    dx0 = ops.conv_bwd(d, x, dy, hwio, dw0, need_dx=True, addend=masked)
    dx1, check, _ = exactref.guarded((n, h, w, CIN), torch.bfloat16, DEV)
    dw1 = torch.full((CIN * COUT,), -7.0, device=DEV)
    got = ops.conv_bwd(d, x, dy, hwio, dw1, need_dx=True, addend=addend, addend_bits=bits, dx=dx1)
    torch.cuda.synchronize()
    assert got.data_ptr() == dx1.data_ptr()
    check('masked-addend dX %s' % (shape,))
    exactref.assert_bits('masked-addend dX %s' % (shape,), dx1.view(torch.int16), dx0.view(torch.int16))
    exactref.assert_bits('masked-addend dW %s' % (shape,), dw1.view(torch.int32), dw0.view(torch.int32))
    # the mask matters: the unmasked addend gives another tensor
    dx2 = ops.conv_bwd(d, x, dy, hwio, dw1, need_dx=True, addend=addend)
    assert not torch.equal(dx2.view(torch.int16), dx0.view(torch.int16))
  finally:
    if knob is not None:
      ops.tune_unset('rowstream')


def test_the_query_keeps_the_measured_row_count():
  """rigl_conv2d_bwd_takes_masked_addend decides at forward time whether the batch norm may skip the masked copy: for the
  row-streaming dgrad from 65 536 rows on (knob "rs_masked_addend" = 2: every legal layer, 0: none); the entry point itself takes
  every layer the kernel is legal for (the test above)."""
  from rigl_amd import ops
  big = ops.conv_desc(16, 64, 64, CIN, COUT, 1, 1, 1, 0, 0, 64, 64)       # 65 536 rows
  small = ops.conv_desc(8, 56, 56, CIN, COUT, 1, 1, 1, 0, 0, 56, 56)      # 25 088 rows
  assert ops.conv_bwd_takes_masked_addend(big) and not ops.conv_bwd_takes_masked_addend(small)
  try:
    ops.tune_set('rs_masked_addend', 2)
    assert ops.conv_bwd_takes_masked_addend(big) and ops.conv_bwd_takes_masked_addend(small)
    ops.tune_set('rs_masked_addend', 0)
    assert not ops.conv_bwd_takes_masked_addend(big) and not ops.conv_bwd_takes_masked_addend(small)
  finally:
    ops.tune_unset('rs_masked_addend')
