"""The masked-layer boundary: ``sparse_conv2d`` / ``sparse_fully_connected``.

Mirrors rigl/imagenet_resnet/pruning_layers.py:72-248 (same argument names,
same ``sparsity_technique`` values, same ValueErrors) on top of the HIP
kernels: ``sparsity_technique='threshold'`` creates `{scope}/weights` and
`{scope}/mask` exactly like contrib's ``masked_conv2d`` (mask initialised to
ones, y = conv(x, mask * W)); ``'baseline'`` creates a dense layer.

Activations are NHWC bf16 tensors ([N,H,W,C] contiguous) -- the reference's
``channels_last`` default and bfloat16 scope (imagenet_train_eval.py:92-98,
549-552).  Weights are fp32 HWIO variables of the graph (variables.py).  The
autograd bridge calls the C ABI: forward = rigl_masked_conv2d_fwd, backward =
rigl_masked_conv2d_dgrad + rigl_masked_conv2d_wgrad; the DENSE dW goes
straight into the layer's slice of the gradient arena (RigL needs it dense,
sparse_optimizers_base.py:478-485) -- there is no PyTorch fallback.
"""
import math
import os

import numpy as np
import torch

from rigl_amd import ops
from rigl_amd import variables as V


def _same_pad(size, k, stride):
  """TF 'SAME': out = ceil(size/stride), pad_total = max((out-1)*s + k - size, 0),
  pad_begin = pad_total // 2 (the extra pixel goes at the end)."""
  out = -(-size // stride)
  total = max((out - 1) * stride + k - size, 0)
  return out, total // 2


def _valid_out(size, k, stride):
  return (size - k) // stride + 1


# RIGL_CONV_PAIR=0: the first block of a group runs projection and conv1 as two autograd nodes (read once; tests override
# the module attribute).
_CONV_PAIR = os.environ.get('RIGL_CONV_PAIR', '1') != '0'


class _HandOver:
  """A gradient handed from one autograd node to the next together with what the receiver needs to finish it.  Both nodes hold
  the object from the forward on: the giver sets ``armed`` where it decides to hand over, calls ``fill(grad, *payload)`` in its
  backward and returns ``grad`` itself; the receiver calls ``take`` on the gradient that arrives.  ``take`` raises where the two
  disagree, or where autograd delivered another tensor (an accumulated or copied gradient): the payload is then not for it."""
  __slots__ = ('armed', 'grad', 'payload')
  knob = did = None        # (the subclass: the switch the messages name; what the giver did when it filled / when it did not)

  def __init__(self):
    self.armed = False
    self.grad = self.payload = None

  def fill(self, grad, *payload):
    self.grad, self.payload = grad, payload

  def take(self, grad):
    """The payload for the receiver's backward, or None for its plain backward (neither side armed).  Empties the holder."""
    filled, payload = self.grad, self.payload
    self.grad = self.payload = None
    if self.armed != (filled is not None):
      raise RuntimeError('%s: the batch norm %s but the forward had decided otherwise' % (self.knob, self.did[filled is None]))
    if filled is None:
      return None
    if grad is not filled and (grad is None or grad.data_ptr() != filled.data_ptr() or grad.shape != filled.shape
                               or not grad.is_contiguous()):
      raise RuntimeError('%s: the gradient that reached the conv is not the one the batch norm handed over' % self.knob)
    return payload


class BnApplyHolder(_HandOver):
  """Between a conv whose backward applies the backward of the batch norm BEHIND it on its dY load
  (ops.conv_bwd_takes_bn_apply) and that batch norm (workloads.nn._FusedBNFn).  Forward: the conv leaves it on its output
  (attribute ``bn_apply``); the batch norm arms it where it will skip its apply pass.  Backward: the batch norm runs
  ops.bn_bwd_reduce, fills (dout; y, bits, saved, coef) and returns dout itself; the conv, one node later, takes them."""
  __slots__ = ()
  knob, did = 'bn_bwd_on_load', ('skipped its apply pass', 'ran its apply pass')


class MaskedAddendHolder(_HandOver):
  """Between relu(bn3 + shortcut) (workloads.nn._FusedBNFn) and the conv whose ``fork`` made the shortcut and whose backward
  masks its addend on the fly (takes_masked_addend).  Forward: ``fork`` leaves it on the alias (attribute ``masked_addend``);
  the batch norm that takes the alias as its residual arms it.  Backward: the batch norm fills (dy; bits) and returns dy itself,
  unmasked, as the residual's gradient; the fork's backward takes the ReLU bits."""
  __slots__ = ()
  knob, did = 'lazy_res_grad', ('handed the shortcut gradient over unmasked', 'wrote the masked shortcut gradient')


def _conv_forward(lv, desc, x, want_stats):
  """(y, statistics or None) of the layer's forward; fp32 activations (--precision=float32) run the validation kernels, which
  have no statistics epilogue."""
  if x.dtype == torch.float32:
    return ops.conv_fwd_f32(desc, x, lv.weights.data.view(-1), _mask_bits(lv)), None
  return ops.conv_fwd(desc, x, lv.ohwi, stats=True) if want_stats else (ops.conv_fwd(desc, x, lv.ohwi), None)


def stats_outputs(ctx, want_stats, outs, parts, device):
  """What a forward returns: ``outs`` (one tensor if it is alone), and with ``want_stats`` the batch-norm statistics ``parts``
  behind them -- an empty tensor where the kernel left none -- as outputs autograd neither differentiates nor zero-fills."""
  if not want_stats:
    return outs if len(outs) > 1 else outs[0]
  parts = tuple(p if p is not None else torch.empty(0, device=device) for p in parts)
  ctx.mark_non_differentiable(*parts)
  ctx.set_materialize_grads(False)
  return outs + parts


def _dw_ready(lv):
  """The callback for "this layer's dW is enqueued": data parallel overlaps its all-reduce from there; None on one GPU."""
  sync = getattr(lv.weights.graph, 'grad_sync', None)
  return (lambda: sync.notify_layer_grad_ready(lv.weights)) if sync is not None else None


def _dy_or_zeros(dy, d, x):
  """The output gradient as the kernels want it; an unused output has a zero gradient."""
  if dy is None:
    return torch.zeros((d.n, d.ho, d.wo, d.cout), dtype=x.dtype, device=x.device)
  return dy.contiguous()


def _mask_bits(lv):
  """The layer's mask bitmap for the fp32 kernels (they read the master weights and apply the mask on the fly)."""
  return lv.mask.bits if lv.mask is not None else None


class _MaskedConvFn(torch.autograd.Function):
  """y = conv(x, mask*W) with dense dW written into lv.weights.grad."""

  @staticmethod
  def forward(ctx, x, lv, desc, need_dx, want_stats=False, pending=None, apply_holder=None):
    ctx.lv, ctx.desc, ctx.need_dx, ctx.apply_holder = lv, desc, need_dx, apply_holder
    ctx.save_for_backward(x)
    if pending is not None:
      # x is the still EMPTY output of a batch norm that only finalised its statistics (workloads.nn.BatchNorm, consumer=):
      # this conv reads the pre-batch-norm tensor, applies scale / shift / ReLU on its operand load and fills x on the way
      out = ops.conv_fwd_bnrelu(desc, pending.x, pending.saved, lv.ohwi, x, stats=want_stats)
      y, part = out if want_stats else (out, None)
    else:
      y, part = _conv_forward(lv, desc, x, want_stats)
    return stats_outputs(ctx, want_stats, (y,), (part,), x.device)

  @staticmethod
  def backward(ctx, dy, _dpart=None):
    (x,) = ctx.saved_tensors
    lv, d = ctx.lv, ctx.desc
    dy = _dy_or_zeros(dy, d, x)
    # dense dL/d(mask*W), fp32 HWIO, into this layer's slice of the G arena, and dX -- one call
    ready = _dw_ready(lv)
    if x.dtype == torch.float32:
      dx = ops.conv_bwd_f32(d, x, dy, lv.weights.data.view(-1), _mask_bits(lv), lv.weights.grad.view(-1),
                            need_dx=ctx.need_dx, on_dw_ready=ready)
      return (dx,) + (None,) * 6
    got = ctx.apply_holder.take(dy) if ctx.apply_holder is not None else None
    if got is not None:
      # dy is the gradient w.r.t. the OUTPUT of the batch norm behind this conv: its apply pass runs on this backward's dY load
      dx = ops.conv_bwd_bnapply(d, x, dy, lv.hwio, lv.weights.grad.view(-1), *got, on_dw_ready=ready)
      return (dx,) + (None,) * 6
    dx = ops.conv_bwd(d, x, dy, lv.hwio, lv.weights.grad.view(-1), need_dx=ctx.need_dx, on_dw_ready=ready)
    return (dx,) + (None,) * 6


class _MaskedConvReluFn(torch.autograd.Function):
  """y = relu(conv(x, mask*W)) with no batch norm in between (VGG: conv2d_fixed_padding + tf.nn.relu, vgg.py:124-134) --
  one node that saves only x; the pre-activation is never stored (rigl_masked_conv2d_fwd_relu).

  Contract of the backward: ``dy`` arrives already gated by [y > 0].  Every consumer of y in a VGG graph does that: the
  next conv of this kind (``gate_input``: its dX is bf16(dgrad) * [x > 0], x = y or a max pool of y -- at the pool winner
  y equals the pooled value), or nn.global_avg_pool_relu.  With ``gate_input`` dX is gated the same way
  (rigl_masked_conv2d_bwd_relu), else it is the plain dgrad (the first conv reads the images and needs none).  Dense dW
  goes into the layer's slice of the gradient arena as for every other layer."""

  @staticmethod
  def forward(ctx, x, lv, desc, need_dx, gate_input):
    ctx.lv, ctx.desc, ctx.need_dx, ctx.gate_input = lv, desc, need_dx, gate_input
    ctx.save_for_backward(x)
    return ops.conv_fwd_relu(desc, x, lv.ohwi)

  @staticmethod
  def backward(ctx, dy):
    (x,) = ctx.saved_tensors
    lv, d = ctx.lv, ctx.desc
    dy, ready = _dy_or_zeros(dy, d, x), _dw_ready(lv)
    if ctx.need_dx and ctx.gate_input:
      dx = ops.conv_bwd_relu(d, x, dy, lv.hwio, lv.weights.grad.view(-1), on_dw_ready=ready)
    else:
      dx = ops.conv_bwd(d, x, dy, lv.hwio, lv.weights.grad.view(-1), need_dx=ctx.need_dx, on_dw_ready=ready)
    return dx, None, None, None, None


class _MaskedConvForkFn(torch.autograd.Function):
  """(y, x') = (conv(x, mask*W), x): the conv plus an alias of its input for the
  tensor's OTHER consumer (a residual shortcut, or the next conv reading the
  same block input).  Backward folds the alias' gradient into the dgrad
  epilogue -- dx = conv2d_backprop_input(dy, mask*W) + dx' -- instead of the
  separate AddN pass autodiff would emit (rigl_masked_conv2d_dgrad_acc)."""

  @staticmethod
  def forward(ctx, x, lv, desc, want_stats=False, addend_holder=None):
    ctx.lv, ctx.desc, ctx.addend_holder = lv, desc, addend_holder
    ctx.save_for_backward(x)
    y, part = _conv_forward(lv, desc, x, want_stats)
    return stats_outputs(ctx, want_stats, (y, x.view_as(x)), (part,), x.device)

  @staticmethod
  def backward(ctx, dy, dalias, _dpart=None):
    (x,) = ctx.saved_tensors
    lv, d = ctx.lv, ctx.desc
    dy, ready = _dy_or_zeros(dy, d, x), _dw_ready(lv)
    if dalias is not None:
      dalias = dalias.contiguous()
    if x.dtype == torch.float32:
      dx = ops.conv_bwd_f32(d, x, dy, lv.weights.data.view(-1), _mask_bits(lv), lv.weights.grad.view(-1),
                            need_dx=True, addend=dalias, on_dw_ready=ready)
      return (dx,) + (None,) * 4
    # the alias' gradient may arrive unmasked with the ReLU bits it still has to pass (workloads.nn._FusedBNFn): only as the very
    # tensor the batch norm handed over -- anything else (autograd summed or copied it) raises instead of being added unmasked
    got = ctx.addend_holder.take(dalias) if ctx.addend_holder is not None else None
    if got is not None:
      dx = ops.conv_bwd(d, x, dy, lv.hwio, lv.weights.grad.view(-1), need_dx=True, addend=dalias, addend_bits=got[0],
                        on_dw_ready=ready)
      return (dx,) + (None,) * 4
    dx = ops.conv_bwd(d, x, dy, lv.hwio, lv.weights.grad.view(-1), need_dx=True, addend=dalias, on_dw_ready=ready)
    return (dx,) + (None,) * 4


class _MaskedConvPairFn(torch.autograd.Function):
  """(y_s, y_m) = (conv_s(x), conv_m(x)): the two readers of a tensor where conv_s is a STRIDED 1x1 conv without padding
  -- the projection shortcut of a ResNet group's first block next to its conv1 (resnet_model.py:456-501).  conv_s only
  reads the pixels (i * sh, j * sw), so dL/dx through it is zero everywhere else.  As two autograd nodes that gradient is
  a full-size tensor (three quarters zeros at stride 2) written by a strided dgrad and read back by the other conv's
  accumulating epilogue; as ONE node it is computed on the [n, ho, wo] grid as the dgrad of a stride-1 1x1 conv and
  handed to conv_m's dgrad epilogue compact (rigl_masked_conv2d_bwd_sub): dx = dgrad_m(dy_m) + scatter(dgrad_s(dy_s)).
  Both dense dW go straight into their gradient-arena slices, as in _MaskedConvFn."""

  @staticmethod
  def forward(ctx, x, lv_s, d_s, lv_m, d_m, want_stats):
    ctx.lv_s, ctx.d_s, ctx.lv_m, ctx.d_m = lv_s, d_s, lv_m, d_m
    ctx.save_for_backward(x)
    ys, ps = _conv_forward(lv_s, d_s, x, want_stats)
    ym, pm = _conv_forward(lv_m, d_m, x, want_stats)
    return stats_outputs(ctx, want_stats, (ys, ym), (ps, pm), x.device)

  @staticmethod
  def backward(ctx, dys, dym, _dps=None, _dpm=None):
    (x,) = ctx.saved_tensors
    lv_s, d_s, lv_m, d_m = ctx.lv_s, ctx.d_s, ctx.lv_m, ctx.d_m
    dys, dym = _dy_or_zeros(dys, d_s, x), _dy_or_zeros(dym, d_m, x)
    # the strided conv: dW from x as it lies; dX on its own grid only (= the dgrad of a stride-1 1x1 conv over that grid)
    dxs = ops.conv_bwd_grid(d_s, x, dys, lv_s.hwio, lv_s.weights.grad.view(-1), on_dw_ready=_dw_ready(lv_s))
    dx = ops.conv_bwd(d_m, x, dym, lv_m.hwio, lv_m.weights.grad.view(-1), need_dx=True, addend=dxs,
                      addend_sub=(d_s.stride_h, d_s.stride_w), on_dw_ready=_dw_ready(lv_m))
    return dx, None, None, None, None, None


def conv_pair(conv_sub, conv_main, x, bn_stats=False):
  """(conv_sub(x), conv_main(x)) for a tensor read by exactly these two convs, conv_sub a strided 1x1 conv (see
  _MaskedConvPairFn); any other pair of layers -- and fp32 activations -- take conv_sub.fork(x) + conv_main(alias)."""
  n, h, w, c = x.shape
  ok = (x.dtype == torch.bfloat16 and x.requires_grad and conv_sub.need_input_grad and conv_main.need_input_grad
        and conv_sub.kh == conv_sub.kw == 1 and max(conv_sub.strides) > 1
        and conv_sub.cin % 8 == 0 and conv_sub.units % 8 == 0 and conv_main.units % 8 == 0
        and _CONV_PAIR)
  d_s = conv_sub.desc_for(n, h, w) if ok else None
  if ok and (d_s.pad_top or d_s.pad_left or d_s.ho != -(-h // d_s.stride_h) or d_s.wo != -(-w // d_s.stride_w)):
    ok = False
  if not ok:
    ys, alias = conv_sub.fork(x, bn_stats)
    return ys, conv_main(alias, bn_stats)
  if c != conv_sub.cin or c != conv_main.cin:
    raise ValueError('expected [N,H,W,%d], got %s' % (conv_sub.cin, tuple(x.shape)))
  conv_sub.graph.refresh_shadows()
  d_m = conv_main.desc_for(n, h, w)
  if not bn_stats:
    return _MaskedConvPairFn.apply(x.contiguous(), conv_sub.vars, d_s, conv_main.vars, d_m, False)
  ys, ym, ps, pm = _MaskedConvPairFn.apply(x.contiguous(), conv_sub.vars, d_s, conv_main.vars, d_m, True)
  if ps.numel():
    ys.bn_partials = ps
  if pm.numel():
    ym.bn_partials = pm
  return ys, ym


class _Layer:
  """Common part of MaskedConv2d / MaskedDense."""

  def __init__(self, graph, scope, shape, sparsity_technique, weight_decay,
               kernel_initializer):
    if sparsity_technique not in ('threshold', 'baseline'):
      raise ValueError(
          'Unsupported sparsity technique {}'.format(sparsity_technique))
    self.graph = graph
    self.scope = scope
    self.masked = sparsity_technique == 'threshold'
    init = kernel_initializer(shape) if kernel_initializer is not None else \
        variance_scaling_initializer()(shape)
    self.vars = graph.add_masked_layer(scope, shape, self.masked, weight_decay,
                                       init)
    self.bias = None

  @property
  def weights(self):
    return self.vars.weights

  @property
  def mask(self):
    return self.vars.mask


class MaskedConv2d(_Layer):
  """masked_conv2d / tf.layers.conv2d twin (pruning_layers.py:139-169)."""

  def __init__(self, graph, scope, cin, units, kernel_size, strides=(1, 1),
               padding='SAME', sparsity_technique='baseline', weight_decay=0.0,
               kernel_initializer=None, need_input_grad=True):
    kh, kw = kernel_size
    super().__init__(graph, scope, (kh, kw, cin, units), sparsity_technique,
                     weight_decay, kernel_initializer)
    if padding not in ('SAME', 'VALID'):
      raise ValueError('padding must be SAME or VALID')
    self.cin, self.units, self.kh, self.kw = cin, units, kh, kw
    self.strides = tuple(strides)
    self.padding = padding
    self.need_input_grad = need_input_grad
    self._descs = {}

  def desc_for(self, n, h, w):
    key = (n, h, w)
    d = self._descs.get(key)
    if d is None:
      sh, sw = self.strides
      if self.padding == 'SAME':
        ho, pt = _same_pad(h, self.kh, sh)
        wo, pl = _same_pad(w, self.kw, sw)
      else:
        ho, pt = _valid_out(h, self.kh, sh), 0
        wo, pl = _valid_out(w, self.kw, sw), 0
      d = ops.conv_desc(n, h, w, self.cin, self.units, self.kh, self.kw,
                        (sh, sw), pt, pl, ho, wo)
      self._descs[key] = d
    return d

  def __call__(self, x, bn_stats=False):
    """``bn_stats``: also leave the batch-norm partial sums of the output on the
    returned tensor (attribute ``bn_partials``) for the BatchNorm that follows,
    which then skips its statistics pass (rigl_masked_conv2d_fwd_stats)."""
    if x.dim() != 4:
      raise ValueError('Rank not supported {}'.format(x.dim()))
    if x.shape[-1] != self.cin:
      raise ValueError('expected %d input channels, got %d' %
                       (self.cin, x.shape[-1]))
    self.graph.refresh_shadows()
    n, h, w, _ = x.shape
    d = self.desc_for(n, h, w)
    need_dx = self.need_input_grad and x.requires_grad
    pending = getattr(x, 'bn_pending', None)   # the batch norm in front left its apply pass to this conv (takes_bn_input)
    if pending is not None and (pending.x is None or not x.is_contiguous()):
      raise RuntimeError('a deferred batch-norm output must reach its consumer conv as it was returned')
    if not x.requires_grad:
      x = x.detach().requires_grad_(True)  # keep the node so wgrad runs
    # the batch norm behind this conv may leave its backward apply pass to this conv's backward (workloads.nn.BatchNorm)
    apply_holder = BnApplyHolder() if (need_dx and x.dtype == torch.bfloat16 and x.is_cuda and ops.conv_bwd_takes_bn_apply(d)) else None
    if not bn_stats:
      y = _MaskedConvFn.apply(x.contiguous(), self.vars, d, need_dx, False, pending, apply_holder)
    else:
      y, part = _MaskedConvFn.apply(x.contiguous(), self.vars, d, need_dx, True, pending, apply_holder)
      if part.numel():
        y.bn_partials = part
    if apply_holder is not None and y.grad_fn is not None:
      y.bn_apply = apply_holder                      # the conv's autograd node and the batch norm that reads y share it
    return y

  def conv_relu(self, x, gate_input=True):
    """relu(conv(x)) as one node (_MaskedConvReluFn; bf16 only).  ``gate_input``: x is a ReLU output (or a max pool of one)
    and dX passes that ReLU's gradient on; the output's own consumer must gate its gradient likewise."""
    if x.dim() != 4 or x.shape[-1] != self.cin:
      raise ValueError('expected [N,H,W,%d], got %s' % (self.cin, tuple(x.shape)))
    if x.dtype != torch.bfloat16:
      raise NotImplementedError('conv_relu: bf16 activations only')
    self.graph.refresh_shadows()
    n, h, w, _ = x.shape
    d = self.desc_for(n, h, w)
    need_dx = self.need_input_grad and x.requires_grad
    if not x.requires_grad:
      x = x.detach().requires_grad_(True)  # keep the node so wgrad runs
    return _MaskedConvReluFn.apply(x.contiguous(), self.vars, d, need_dx, bool(gate_input))

  def takes_bn_input(self, x):
    """Does this conv's forward take relu(bn(.)) of its input on its operand load (rigl_masked_conv2d_fwd_bnrelu)?  ``x`` = the
    batch norm's input (the shape of this conv's input)."""
    if not (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 4 and x.shape[-1] == self.cin):
      return False
    n, h, w, _ = x.shape
    return ops.conv_fwd_takes_bn_input(self.desc_for(n, h, w))

  def takes_masked_addend(self, x):
    """Can the gradient of ``fork(x)``'s alias be handed to this conv unmasked with a 1-bit mask (rigl_masked_conv2d_bwd_masked)?
    Only then may the alias' other consumer (relu(bn3 + alias)) skip writing the masked gradient."""
    if not (self.need_input_grad and x.requires_grad and x.dtype == torch.bfloat16 and x.dim() == 4):
      return False
    n, h, w, _ = x.shape
    return ops.conv_bwd_takes_masked_addend(self.desc_for(n, h, w))

  def fork(self, x, bn_stats=False):
    """Returns (conv(x), x'): use x' for x's other consumer and its gradient
    is accumulated inside this conv's dgrad kernel (see _MaskedConvForkFn)."""
    if x.dim() != 4 or x.shape[-1] != self.cin:
      raise ValueError('expected [N,H,W,%d], got %s' % (self.cin, tuple(x.shape)))
    if not (self.need_input_grad and x.requires_grad):
      return self(x, bn_stats), x
    self.graph.refresh_shadows()
    n, h, w, _ = x.shape
    # relu(bn + alias) may hand the alias' gradient back unmasked with the ReLU bits (workloads.nn.BatchNorm arms this)
    addend_holder = MaskedAddendHolder() if self.takes_masked_addend(x) else None
    y, alias, *part = _MaskedConvForkFn.apply(x.contiguous(), self.vars, self.desc_for(n, h, w), bn_stats, addend_holder)
    if part and part[0].numel():
      y.bn_partials = part[0]
    if addend_holder is not None:
      alias.masked_addend = addend_holder
    return y, alias


class MaskedDense(_Layer):
  """masked_fully_connected / tf.layers.dense twin (pruning_layers.py:222-245):
  y = x @ (mask*W) + b, weights [in, out]; runs as a 1x1 conv."""

  def __init__(self, graph, scope, n_in, units, use_bias=True,
               sparsity_technique='baseline', weight_decay=0.0,
               kernel_initializer=None, activation=None):
    super().__init__(graph, scope, (n_in, units), sparsity_technique,
                     weight_decay, kernel_initializer)
    self.n_in, self.units = n_in, units
    self.activation = activation
    self._descs = {}
    if use_bias:
      self.bias = graph.add_variable(scope + '/biases', (units,), V.KIND_OTHER, 0.0)

  def __call__(self, x):
    if x.shape[-1] != self.n_in:
      raise ValueError('expected %d inputs, got %d' % (self.n_in, x.shape[-1]))
    self.graph.refresh_shadows()
    lead = x.shape[:-1]
    x2 = x.reshape(-1, 1, 1, self.n_in)
    b = x2.shape[0]
    d = self._descs.get(b)
    if d is None:
      d = ops.conv_desc(b, 1, 1, self.n_in, self.units, 1, 1, 1, 0, 0, 1, 1)
      self._descs[b] = d
    need_dx = x2.requires_grad
    if not x2.requires_grad:
      x2 = x2.detach().requires_grad_(True)
    y = _MaskedConvFn.apply(x2.contiguous(), self.vars, d, need_dx)
    y = y.reshape(*lead, self.units)
    if self.bias is not None:
      y = y + bias_tensor(self.bias).to(y.dtype)
    if self.activation is not None:
      y = self.activation(y)
    return y


def bias_tensor(var):
  """An autograd leaf aliasing the variable's storage whose .grad IS the
  variable's slice of the gradient arena (autograd accumulates in place).
  The variable's own ``data`` tensor never requires grad, so the arenas stay
  outside any autograd graph; the kernels update them in place."""
  leaf = getattr(var, '_leaf', None)
  if leaf is None or leaf.data_ptr() != var.data.data_ptr():
    leaf = var.data.detach().requires_grad_(True)
    var._leaf = leaf
  if leaf.grad is None or leaf.grad.data_ptr() != var.grad.data_ptr():
    leaf.grad = var.grad
  return leaf


# ----------------------------------------------------------------------------
# initializers (host side, NumPy; shapes are HWIO / [in, out])
# ----------------------------------------------------------------------------
_init_rng = np.random.RandomState(0)


def set_init_seed(seed):
  global _init_rng
  _init_rng = np.random.RandomState(seed)


def variance_scaling_initializer(scale=1.0):
  """tf.variance_scaling_initializer(scale): fan_in, truncated normal
  (resnet_model.py:283)."""

  def init(shape):
    fan_in = int(np.prod(shape[:-1]))
    std = math.sqrt(scale / max(1.0, fan_in)) / .87962566103423978
    v = _init_rng.randn(*shape)
    bad = np.abs(v) > 2
    while bad.any():
      v[bad] = _init_rng.randn(int(bad.sum()))
      bad = np.abs(v) > 2
    return (v * std).astype(np.float32)

  return init


def random_normal_initializer(stddev=0.01):
  return lambda shape: (_init_rng.randn(*shape) * stddev).astype(np.float32)


# ----------------------------------------------------------------------------
# the reference's functional API
# ----------------------------------------------------------------------------
def _regularizer_scale(reg):
  """kernel_regularizer may be a float (l2 scale) or an object with .scale."""
  if reg is None:
    return 0.0
  if isinstance(reg, (int, float)):
    return float(reg)
  return float(getattr(reg, 'scale'))


class l2_regularizer:  # pylint: disable=invalid-name
  """contrib_layers.l2_regularizer(scale): scale * sum(w^2) / 2; its gradient
  (scale * w) is applied inside the fused update kernel (K3)."""

  def __init__(self, scale):
    self.scale = float(scale)


def sparse_conv2d(x, units, kernel_size, activation=None, use_bias=False,
                  kernel_initializer=None, kernel_regularizer=None,
                  bias_initializer=None, biases_regularizer=None,
                  sparsity_technique='baseline', normalizer_fn=None,
                  strides=(1, 1), padding='SAME', data_format='channels_last',
                  name=None, graph=None):
  """rigl/imagenet_resnet/pruning_layers.py:72-172.  Variables are created on
  the first call for a scope and reused afterwards (tf.variable_scope)."""
  del bias_initializer, biases_regularizer
  if data_format == 'channels_last':
    pass
  elif data_format == 'channels_first':
    raise ValueError('channels_first is not supported by the NHWC kernels')
  else:
    raise ValueError('Not a valid channel string:', data_format)
  if x.dim() != 4:
    raise ValueError('Rank not supported {}'.format(x.dim()))
  if sparsity_technique not in ('threshold', 'baseline'):
    raise ValueError(
        'Unsupported sparsity technique {}'.format(sparsity_technique))
  if use_bias:
    raise ValueError('use_bias=True is not used by the reference models')
  g = graph or V.get_default_graph()
  key = name
  layer = g.modules.get(key) if key is not None else None
  if layer is None:
    scope = g.unique_scope(name, 'Conv')
    layer = MaskedConv2d(g, scope, x.shape[-1], units, tuple(kernel_size),
                         tuple(strides), padding, sparsity_technique,
                         _regularizer_scale(kernel_regularizer),
                         kernel_initializer)
    g.modules[scope] = layer
  y = layer(x)
  if normalizer_fn is not None:
    y = normalizer_fn(y)
  if activation is not None:
    y = activation(y)
  return y


def sparse_fully_connected(x, units, activation=None, use_bias=True,
                           kernel_initializer=None, kernel_regularizer=None,
                           bias_initializer=None, biases_regularizer=None,
                           sparsity_technique='baseline', name=None,
                           graph=None):
  """rigl/imagenet_resnet/pruning_layers.py:175-248."""
  del bias_initializer, biases_regularizer
  if sparsity_technique not in ('threshold', 'baseline'):
    raise ValueError(
        'Unsupported sparsity technique {}'.format(sparsity_technique))
  g = graph or V.get_default_graph()
  layer = g.modules.get(name) if name is not None else None
  if layer is None:
    scope = g.unique_scope(name, 'Dense')
    layer = MaskedDense(g, scope, x.shape[-1], units, use_bias,
                        sparsity_technique,
                        _regularizer_scale(kernel_regularizer),
                        kernel_initializer, activation)
    g.modules[scope] = layer
  return layer(x)
