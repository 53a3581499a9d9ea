"""The fp64 references of tests/convref.py pinned on the host: depthwise_fp64 (per-tap elementwise products + autograd)
against a grouped fp64 F.conv2d on explicitly padded NCHW tensors, per element to 1e-12 of sum |a||b|, at the padding
and stride rules of the workloads (stride 1 SAME, stride 2 fixed padding 1/1 + VALID, TF SAME (0, 1)) on odd sizes.
The GPU parity tests take this reference as ground truth, so it has to be right without a GPU."""
import pytest

torch = pytest.importorskip('torch')
import torch.nn.functional as F  # noqa: E402

from tests import convref  # noqa: E402


def _grouped_fp64(x, w, dy, stride, pads):
  """x [N,H,W,C], w [kh,kw,C], dy [N,Ho,Wo,C]; pads = (top, left, bottom, right) -> y, dx, dw in the same layouts."""
  C = x.shape[-1]
  pt, pl, pb, pr = pads
  xr = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
  wr = w.double().permute(2, 0, 1).unsqueeze(1).contiguous().requires_grad_(True)       # [C, 1, kh, kw]
  y = F.conv2d(F.pad(xr, (pl, pr, pt, pb)), wr, stride=stride, groups=C)
  y.backward(dy.double().permute(0, 3, 1, 2))
  return y.detach().permute(0, 2, 3, 1), xr.grad.permute(0, 2, 3, 1), wr.grad[:, 0].permute(1, 2, 0)


# N, H, W, C, k, stride, pad_top, pad_left, Ho, Wo
CASES = [
    (2, 7, 9, 8, 3, 1, 1, 1, 7, 9),          # stride 1 SAME
    (3, 15, 13, 16, 3, 2, 1, 1, 8, 7),       # stride 2, fixed padding 1 / 1 + VALID (the MobileNet-v1 rule), odd sizes
    (2, 9, 11, 24, 3, 2, 1, 1, 5, 6),        # ... again, the last column needs the right padding
    (2, 5, 7, 8, 3, 2, 1, 1, 3, 4),          # ... a tiny odd plane
    (2, 16, 12, 8, 3, 2, 0, 0, 8, 6),        # TF SAME at stride 2 on an even plane: pad (0, 1)
    (1, 15, 12, 8, 3, 2, 1, 0, 8, 6),        # TF SAME on an odd height (1, 1) and an even width (0, 1)
    (2, 11, 9, 8, 5, 1, 2, 2, 11, 9),        # 5x5 stride 1 SAME
]


@pytest.mark.parametrize('case', CASES)
def test_depthwise_fp64_matches_grouped_conv2d(case):
  N, H, W, C, k, s, pt, pl, Ho, Wo = case
  pb = max((Ho - 1) * s + k - H - pt, 0)
  pr = max((Wo - 1) * s + k - W - pl, 0)
  g = torch.Generator().manual_seed(sum(case))
  x = torch.randn(N, H, W, C, generator=g, dtype=torch.float64)
  w = torch.randn(k, k, C, generator=g, dtype=torch.float64)
  dy = torch.randn(N, Ho, Wo, C, generator=g, dtype=torch.float64)
  ref = convref.depthwise_fp64(x, w, dy, s, pt, pl, Ho, Wo)
  ab = convref.depthwise_fp64(x.abs(), w.abs(), dy.abs(), s, pt, pl, Ho, Wo)
  y, dx, dw = _grouped_fp64(x, w, dy, s, (pt, pl, pb, pr))
  assert ref['y'].shape == (N, Ho, Wo, C) and ref['dx'].shape == (N, H, W, C) and ref['dw'].shape == (k, k, C)
  assert all(t.dtype == torch.float64 for t in ref.values())
  convref.check_close('y', ref['y'], y, ab['y'], 1e-12)
  convref.check_close('dx', ref['dx'], dx, ab['dx'], 1e-12)
  convref.check_close('dw', ref['dw'], dw, ab['dw'], 1e-12)
  # the bounds' sum |a||b| is the same reference on the magnitudes: positive wherever a tap lands
  assert bool((ab['y'] > 0).all()) and bool((ab['dw'] > 0).all())


def test_depthwise_fp64_takes_hwc1_weights_bf16_operands_and_subsets():
  """The [kh,kw,C,1] layout of the depthwise variables, bf16 operands (widened exactly), and want= without dx / dw."""
  g = torch.Generator().manual_seed(5)
  x = torch.randn(2, 9, 7, 16, generator=g).to(torch.bfloat16)
  w = (torch.randn(3, 3, 16, 1, generator=g) * 0.3).to(torch.bfloat16)
  dy = torch.randn(2, 5, 4, 16, generator=g).to(torch.bfloat16)
  full = convref.depthwise_fp64(x, w, dy, 2, 1, 1, 5, 4)
  y, dx, dw = _grouped_fp64(x, w.reshape(3, 3, 16), dy, 2, (1, 1, 1, 1))
  assert float((full['y'] - y).abs().max()) <= 1e-12 * float(y.abs().max())
  assert float((full['dw'] - dw).abs().max()) <= 1e-12 * float(dw.abs().max())
  assert float((full['dx'] - dx).abs().max()) <= 1e-12 * float(dx.abs().max())
  only_y = convref.depthwise_fp64(x, w, dy, 2, 1, 1, 5, 4, want=('y',))
  assert set(only_y) == {'y'} and torch.equal(only_y['y'], full['y'])
  no_dx = convref.depthwise_fp64(x, w, dy, 2, 1, 1, 5, 4, want=('y', 'dw'))
  assert set(no_dx) == {'y', 'dw'} and torch.equal(no_dx['dw'], full['dw'])


def test_depthwise_fp64_catches_a_wrong_channel():
  """The check has teeth: one channel of dW scaled by 1 + 2^-20 is far outside 1e-12 of sum |x||dy|."""
  g = torch.Generator().manual_seed(9)
  x = torch.randn(2, 7, 7, 8, generator=g, dtype=torch.float64)
  w = torch.randn(3, 3, 8, generator=g, dtype=torch.float64)
  dy = torch.randn(2, 7, 7, 8, generator=g, dtype=torch.float64)
  ref = convref.depthwise_fp64(x, w, dy, 1, 1, 1, 7, 7)
  ab = convref.depthwise_fp64(x.abs(), w.abs(), dy.abs(), 1, 1, 1, 7, 7)
  bad = ref['dw'].clone()
  bad[:, :, 5] *= 1 + 2.0 ** -20
  with pytest.raises(AssertionError):
    convref.check_close('dw', bad, ref['dw'], ab['dw'], 1e-12)
