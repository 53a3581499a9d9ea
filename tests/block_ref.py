"""Stock-op float64 twins of the network BLOCKS -- TEST INFRASTRUCTURE, never imported by the product.

Every kernel of the library is pinned on its own; these twins state what a whole block computes, so that the code that
wires the kernels together (workloads/resnet50.py::_Bottleneck, workloads/mobilenet_v1.py, the autograd bridge of
pruning_layers.py and workloads/nn.py) can be held to something that is not itself.  The mathematics is the reference
model definitions' (rigl/imagenet_resnet/resnet_model.py: fixed_padding :83-108, conv2d_fixed_padding :234-303,
bottleneck_block_ :396-501, the stem :612-644, the head :701-716; mobilenetv1_model.py: depthwise_conv2d_fixed_padding
:43-92, mbv1_block_ :156-220; imagenet_train_eval.py:578-584 for the loss), written with torch.nn.functional and
autograd -- not the product's wiring: no fork, no pair node, no hand-over, one autograd graph per block.

Rounding points (``rounding=True``).  A value is rounded to bf16 in the forward, and its gradient in the backward,
wherever the HIP path stores a bf16 tensor or a fused kernel reproduces one (include/rigl_hip.h, workloads/nn.py):
  * every conv output (and with it the gradient a batch norm's backward stores for the conv in front of it; where that
    apply pass runs on the conv's dY load the kernel forms the same bf16 value in registers);
  * every relu(bn(.)) output (and with it the bf16 dgrad of the conv that reads it);
  * the normalised projection shortcut inside bn_add_bn ("rounds the shortcut to bf16 where bn2 alone would have stored
    it"), and relu(bn3 + shortcut);
  * bf16(bf16(dgrad) + addend) where a tensor has two readers: each reader's input gradient is rounded, then the sum;
  * the projection's compact input gradient before it is scattered (rigl_masked_conv2d_bwd_grid);
  * the max pool's input gradient (rigl_maxpool_bwd stores it; the fused stem tail gathers the same rounded value);
  * the pooled features, the logits before and after the bias, the bf16 copy of the bias and of its gradient, dlogits;
  * the weight operands: bf16(mask * W).  Depthwise weights are read as fp32 and are NOT rounded.
``rounding=False`` is the plain function of the unrounded operands.  ``dtype`` is the arithmetic: float64, or float32
for the noise floor of the comparison (what fp32 accumulation alone costs against float64, reference code only).

Layouts are the product's: activations [N, H, W, C], conv weights HWIO, depthwise weights [kh, kw, C, 1], dense weights
[in, out].  Every twin returns a dict of detached ``dtype`` tensors: ``y`` (the block output), ``dx`` (absent where the
segment has no input gradient), ``dw_<conv>`` = the DENSE gradient w.r.t. mask * W, ``dgamma_<bn>`` / ``dbeta_<bn>``.
"""
import torch
import torch.nn.functional as F

from tests import glue_ref

BN_EPS = 1e-5                       # resnet_model.py:38
BOUND = 2.0**-6                     # relative L2 per compared tensor, see bound_note
OUTER_REL, OUTER_NORM = 0.15, 0.05  # tests/test_network_grad_gpu.py's chain bound: no case may leave it under any explanation

bound_note = """relative L2 <= 2^-6 per compared tensor against the rounding-point float64 twin: two correct bf16
implementations may round any stored element the other way, at most 2^-8 relative per element and so at most 2^-8
relative L2 per stored tensor; fewer than eight stored tensors lie between any input and any output of these blocks;
adding linearly, 8 * 2^-9 = 2^-6.  A tensor whose reference norm is zero must be exactly zero."""


class _RoundBF16(torch.autograd.Function):
  """bf16 rounding of a tensor in the forward AND of its gradient in the backward pass, in any arithmetic dtype."""

  @staticmethod
  def forward(ctx, x):
    return x.to(torch.bfloat16).to(x.dtype)

  @staticmethod
  def backward(ctx, g):
    return g.to(torch.bfloat16).to(g.dtype)


def rounder(rounding):
  return _RoundBF16.apply if rounding else (lambda t: t)


def rel_l2(got, ref):
  """||got - ref|| / ||ref|| in float64; a reference of norm zero admits only an exactly zero tensor (-> 0.0, else inf)."""
  got, ref = got.detach().double(), ref.detach().double()
  assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
  den = float(ref.norm())
  if den == 0.0:
    return 0.0 if not bool(got.any()) else float('inf')
  return float((got - ref).norm()) / den


# ---------------------------------------------------------------------------------------------------------------------
# pieces (NCHW inside)
# ---------------------------------------------------------------------------------------------------------------------
def nchw(x_nhwc, dtype):
  return x_nhwc.detach().to(dtype).permute(0, 3, 1, 2).contiguous()


def nhwc(t):
  return t.detach().permute(0, 2, 3, 1).contiguous()


def leaf(t):
  return t.detach().clone().requires_grad_(True)


def conv_weight(w_hwio, dtype, rounding):
  """The leaf the dense dW is taken against: mask * W as the kernels read it (the bf16 shadow), OIHW inside."""
  w = w_hwio.detach()
  if rounding:
    w = w.to(torch.bfloat16)
  return leaf(w.to(dtype).permute(3, 2, 0, 1).contiguous())


def hwio(w_oihw_grad):
  return w_oihw_grad.detach().permute(2, 3, 1, 0).contiguous()


def fixed_padding(x, k):
  """resnet_model.fixed_padding: (k - 1) // 2 in front, the rest behind, whatever the input size."""
  beg = (k - 1) // 2
  end = k - 1 - beg
  return F.pad(x, (beg, end, beg, end))


def same_padding(x, k, stride):
  """tf 'SAME': out = ceil(size / stride), the smaller half of the padding in front."""
  h, w = x.shape[2], x.shape[3]
  th = max((-(-h // stride) - 1) * stride + k - h, 0)
  tw = max((-(-w // stride) - 1) * stride + k - w, 0)
  return F.pad(x, (tw // 2, tw - tw // 2, th // 2, th - th // 2))


def conv2d_fixed_padding(x, w_oihw, stride):
  """conv2d_fixed_padding: stride > 1 pads explicitly and convolves 'VALID', stride 1 convolves 'SAME'."""
  k = w_oihw.shape[-1]
  x = fixed_padding(x, k) if stride > 1 else same_padding(x, k, 1)
  return F.conv2d(x, w_oihw, stride=stride)


def depthwise_conv2d_fixed_padding(x, w_c1hw, stride):
  k = w_c1hw.shape[-1]
  x = fixed_padding(x, k) if stride > 1 else same_padding(x, k, 1)
  return F.conv2d(x, w_c1hw, stride=stride, groups=w_c1hw.shape[0])


def batch_norm(x, gamma, beta):
  """tf.layers.batch_normalization in training mode: batch statistics, biased variance."""
  return F.batch_norm(x, None, None, gamma, beta, True, 0.1, BN_EPS)


class _MaxPoolFirstMax(torch.autograd.Function):
  """Max pooling (NCHW) with the tie rule tests/glue_ref.py states and tests/test_pool_gpu.py pins: taps outside the
  image take no part, the FIRST maximum in row-major window order wins and receives the whole gradient."""

  @staticmethod
  def forward(ctx, x, d):
    shape = (d.n, d.cin, d.ho, d.wo)
    best = torch.zeros(shape, dtype=x.dtype, device=x.device)
    has = torch.zeros(shape, dtype=torch.bool, device=x.device)
    arg = torch.zeros(shape, dtype=torch.uint8, device=x.device)
    for r in range(d.kh):
      for s in range(d.kw):
        rg = glue_ref._tap_ranges(d, r, s)  # pylint: disable=protected-access
        if rg is None:
          continue
        oh, ow, ih, iw = rg
        v = x[:, :, ih, iw]
        take = ~has[:, :, oh, ow] | (v > best[:, :, oh, ow])
        best[:, :, oh, ow] = torch.where(take, v, best[:, :, oh, ow])
        arg[:, :, oh, ow] = torch.where(take, torch.full_like(arg[:, :, oh, ow], r * d.kw + s), arg[:, :, oh, ow])
        has[:, :, oh, ow] |= take
    ctx.d = d
    ctx.save_for_backward(arg)
    return best

  @staticmethod
  def backward(ctx, dy):
    d, (arg,) = ctx.d, ctx.saved_tensors
    dx = torch.zeros((d.n, d.cin, d.h, d.w), dtype=dy.dtype, device=dy.device)
    for r in range(d.kh):
      for s in range(d.kw):
        rg = glue_ref._tap_ranges(d, r, s)  # pylint: disable=protected-access
        if rg is None:
          continue
        oh, ow, ih, iw = rg
        dx[:, :, ih, iw] += torch.where(arg[:, :, oh, ow] == r * d.kw + s, dy[:, :, oh, ow], torch.zeros_like(dy[:, :, oh, ow]))
    return dx, None


def max_pool_3x3_s2_same(x):
  """tf.layers.max_pooling2d(3, 2, 'SAME') (resnet_model.py:637-644)."""
  n, c, h, w = x.shape
  return _MaxPoolFirstMax.apply(x, glue_ref.same_pool_desc(n, h, w, c, 3, 2))


def softmax_cross_entropy(logits, labels, label_smoothing):
  """tf.losses.softmax_cross_entropy(onehot, logits, label_smoothing): targets onehot * (1 - eps) + eps / K, batch mean."""
  logp = F.log_softmax(logits, dim=-1)
  k = logits.shape[-1]
  t = torch.full_like(logp, label_smoothing / k)
  t.scatter_add_(1, labels.reshape(-1, 1), torch.full_like(logp[:, :1], 1.0 - label_smoothing))
  return -(t * logp).sum(dim=1).mean()


def _bn_leaves(bn, dtype):
  return {k: (leaf(g.to(dtype)), leaf(b.to(dtype))) for k, (g, b) in bn.items()}


def _collect(out, convs, bns):
  for k, w in convs.items():
    out['dw_' + k] = hwio(w.grad)
  for k, (g, b) in bns.items():
    out['dgamma_' + k], out['dbeta_' + k] = g.grad.detach(), b.grad.detach()
  return out


# ---------------------------------------------------------------------------------------------------------------------
# the blocks
# ---------------------------------------------------------------------------------------------------------------------
def bottleneck(x, dy, w, bn, stride=1, dtype=torch.float64, rounding=True):
  """bottleneck_block_: ``w`` = {'c1', 'c2', 'c3' (, 'proj')}: mask * W fp32 HWIO; ``bn`` = {'bn1', 'bn2', 'bn3'
  (, 'bn_proj')}: (gamma, beta); a projection shortcut where 'proj' is given, ``stride`` on the 3x3 and the projection."""
  r = rounder(rounding)
  W = {k: conv_weight(v, dtype, rounding) for k, v in w.items()}
  B = _bn_leaves(bn, dtype)
  x0 = leaf(nchw(x, dtype))
  inputs = r(x0)                                             # dX: the stored sum of its two readers' gradients
  shortcut = inputs
  if 'proj' in W:
    shortcut = r(conv2d_fixed_padding(r(inputs), W['proj'], stride))       # (its input gradient is stored before it is added)
    shortcut = r(batch_norm(shortcut, *B['bn_proj']))
  h = r(conv2d_fixed_padding(r(inputs), W['c1'], 1))
  h = r(F.relu(batch_norm(h, *B['bn1'])))
  h = r(conv2d_fixed_padding(h, W['c2'], stride))
  h = r(F.relu(batch_norm(h, *B['bn2'])))
  h = r(conv2d_fixed_padding(h, W['c3'], 1))
  y = r(F.relu(batch_norm(h, *B['bn3']) + shortcut))
  y.backward(nchw(dy, dtype))
  return _collect({'y': nhwc(y), 'dx': nhwc(x0.grad)}, W, B)


def mobilenet_block(x, dy, w_dw, w_pw, bn, stride=1, dtype=torch.float64, rounding=True):
  """mbv1_block_: depthwise 3x3 (``w_dw`` fp32 [3, 3, C, 1], read as it is) -> BN-ReLU -> masked 1x1 (``w_pw``) -> BN-ReLU;
  ``bn`` = {'bn_a', 'bn_b'}."""
  r = rounder(rounding)
  Wd = leaf(w_dw.detach().to(dtype).permute(2, 3, 0, 1).contiguous())     # [C, 1, kh, kw]
  W = {'pw': conv_weight(w_pw, dtype, rounding)}
  B = _bn_leaves(bn, dtype)
  x0 = leaf(nchw(x, dtype))
  h = r(depthwise_conv2d_fixed_padding(r(x0), Wd, stride))
  h = r(F.relu(batch_norm(h, *B['bn_a'])))
  h = r(conv2d_fixed_padding(h, W['pw'], 1))
  y = r(F.relu(batch_norm(h, *B['bn_b'])))
  y.backward(nchw(dy, dtype))
  out = _collect({'y': nhwc(y), 'dx': nhwc(x0.grad)}, W, B)
  out['dw_dw'] = Wd.grad.detach().permute(2, 3, 0, 1).contiguous()
  return out


def resnet_stem(x, dy, w, bn, dtype=torch.float64, rounding=True):
  """7x7 / 2 conv2d_fixed_padding -> batch_norm_relu -> max_pooling2d(3, 2, 'SAME'); the images get no gradient.
  ``bn`` = {'bn': (gamma, beta)}."""
  r = rounder(rounding)
  W = {'stem': conv_weight(w, dtype, rounding)}
  B = _bn_leaves(bn, dtype)
  h = r(conv2d_fixed_padding(nchw(x, dtype), W['stem'], 2))
  h = r(F.relu(batch_norm(h, *B['bn'])))
  y = max_pool_3x3_s2_same(h)
  y.backward(nchw(dy, dtype))
  return _collect({'y': nhwc(y)}, W, B)


def head(x, labels, w, bias, label_smoothing, dtype=torch.float64, rounding=True):
  """Global average pool -> masked dense with bias (``w`` = mask * W fp32 [in, out]) -> label-smoothed cross entropy,
  batch mean.  ``y`` is the loss (a 0-d tensor)."""
  r = rounder(rounding)
  wl = w.detach()
  if rounding:
    wl = wl.to(torch.bfloat16)
  wl = leaf(wl.to(dtype))
  b = leaf(bias.detach().to(dtype))
  x0 = leaf(x.detach().to(dtype))                             # NHWC
  feat = r(r(x0).mean(dim=(1, 2)))
  logits = r(r(feat @ wl) + r(b))
  loss = softmax_cross_entropy(logits, labels, label_smoothing)
  loss.backward()
  return {'y': loss.detach(), 'dx': x0.grad.detach(), 'dw_fc': wl.grad.detach(), 'dbias': b.grad.detach()}
