"""VGG-A / VGG-16 / VGG-19 workloads (rigl/imagenet_resnet/vgg.py:57-251).

Five stages of 3x3 / stride-1 / SAME convs without bias (conv2d_fixed_padding, resnet_model.py:234-303), each followed by
a ReLU and no batch norm; a 2x2/2 VALID max pool after stages 1-4; the spatial mean (global_pool=True); fc8, a masked 1x1
conv to num_classes without bias or ReLU, squeezed to [N, num_classes].  He initialisation (variance_scaling, scale 2.0,
vgg.py:120) and l2 weight decay on every kernel, fc8 included.

Every conv + ReLU is one autograd node (pruning_layers.MaskedConv2d.conv_relu): the ReLU runs in the conv's forward
epilogue, and the ReLU's gradient is applied by the consumer -- the next conv's dgrad epilogue gates dX by [x > 0] (x is
the ReLU output or its max pool), the last one by the average pool's backward.  Activations NHWC bf16 only.
"""
import numpy as np
import torch

from rigl_amd import ops
from rigl_amd import pruning_layers as PL
from rigl_amd import variables as V
from rigl_amd.workloads import nn as gnn
from rigl_amd.workloads import shapes as WS

_LIMIT_ELEMS = (1 << 30) - 1   # the conv bodies address bf16 tensors with 32-bit byte offsets (rigl_hip.h: RIGL_EUNSUPPORTED)


def _glorot_uniform(shape):
  """layers.conv2d's default xavier_initializer (uniform) for the unpruned fc8 (vgg.py:192-193)."""
  fan_in, fan_out = int(np.prod(shape[:-1])), int(np.prod(shape[:-2])) * shape[-1]
  lim = np.sqrt(6.0 / (fan_in + fan_out))
  return PL._init_rng.uniform(-lim, lim, size=shape).astype(np.float32)   # pylint: disable=protected-access


class VGG:

  def __init__(self, vgg_type='vgg_16', num_classes=1000, pruning_method='threshold', prune_last_layer=True, width=1.0,
               weight_decay=0.0, seed=0, graph=None, init_method='baseline', precision='bfloat16'):
    if init_method != 'baseline':
      raise NotImplementedError('init_method %r: only the baseline initialisation is implemented' % init_method)
    if precision not in (None, 'bfloat16'):
      raise NotImplementedError('VGG runs bf16 activations only (precision %r)' % precision)
    if vgg_type not in WS.VGG_CFG:
      raise ValueError('unknown VGG type %r (one of %s)' % (vgg_type, sorted(WS.VGG_CFG)))
    for f in WS.VGG_STAGE_FILTERS:
      if int(f * width) <= 0 or int(f * width) % 8:
        raise ValueError('width %g gives %d channels: the conv bodies need a positive multiple of 8' % (width, int(f * width)))
    self.vgg_type, self.num_classes, self.width = vgg_type, num_classes, width
    self.graph = g = graph or V.get_default_graph()
    PL.set_init_seed(seed)
    self.convs = []          # (MaskedConv2d, stage)
    stages = [int(n.split('/')[1][4:]) for n, _, _ in WS.vgg_convs(vgg_type, width)]
    for k, ((name, cin, cout), st) in enumerate(zip(WS.vgg_convs(vgg_type, width), stages)):
      conv = PL.MaskedConv2d(g, name, cin, cout, (3, 3), (1, 1), 'SAME', pruning_method, weight_decay,
                             PL.variance_scaling_initializer(2.0), need_input_grad=k > 0)
      g.modules[name] = conv
      self.convs.append((conv, st))
    c = self.convs[-1][0].units
    fc8 = vgg_type + '/fc8'
    if prune_last_layer:
      self.fc = PL.MaskedConv2d(g, fc8, c, num_classes, (1, 1), (1, 1), 'SAME', pruning_method, weight_decay,
                                PL.variance_scaling_initializer(2.0))
      self.fc_dense = False
    else:                    # layers.conv2d: unmasked, with bias, xavier init, no regulariser
      self.fc = PL.MaskedDense(g, fc8, c, num_classes, True, 'baseline', 0.0, _glorot_uniform)
      self.fc_dense = True
    g.modules[fc8] = self.fc
    g.finalize()
    self._pool_descs = {}

  # ---- geometry checks -------------------------------------------------------------------------------------------------
  def _check_input(self, images):
    if images.dim() != 4 or images.shape[-1] != 3:
      raise ValueError('images must be [N, H, W, 3] NHWC, got %s' % (tuple(images.shape),))
    if images.dtype != torch.bfloat16:
      raise NotImplementedError('VGG runs bf16 activations only (got %s)' % images.dtype)
    n, h, w, _ = images.shape
    if h % 16 or w % 16:
      raise ValueError('VGG needs H and W divisible by 16 (four 2x2 pools), got %dx%d' % (h, w))
    for conv, st in self.convs:
      s = 2**(st - 1)
      if n * (h // s) * (w // s) * max(conv.cin, conv.units) > _LIMIT_ELEMS:
        raise ValueError('batch %d at %dx%d: %s has a tensor of >= 2^30 elements, beyond the conv bodies\' 32-bit '
                         'addressing; use a smaller batch' % (n, h, w, conv.scope))

  def _pool_desc(self, x):
    n, h, w, c = x.shape
    key = (n, h, w, c)
    d = self._pool_descs.get(key)
    if d is None:
      d = self._pool_descs[key] = ops.conv_desc(n, h, w, c, c, 2, 2, 2, 0, 0, h // 2, w // 2)   # layers.max_pool2d: 2x2/2 VALID
    return d

  def _fc8(self, pooled):
    if self.fc_dense:
      return self.fc(pooled)
    return self.fc(pooled.reshape(pooled.shape[0], 1, 1, -1)).reshape(pooled.shape[0], self.num_classes)

  # ---- training forward ------------------------------------------------------------------------------------------------
  def __call__(self, images, is_training=True):
    """Logits [N, num_classes] (bf16).  ``is_training`` changes nothing: VGG has no batch norm or dropout here."""
    del is_training
    self._check_input(images)
    x, prev = images, 1
    for k, (conv, st) in enumerate(self.convs):
      if st != prev:
        x = gnn._MaxPoolFn.apply(x, self._pool_desc(x))   # pylint: disable=protected-access
        prev = st
      x = conv.conv_relu(x, gate_input=k > 0)
    return self._fc8(gnn.global_avg_pool_relu(x))

  def loss(self, images, labels, label_smoothing=0.1, is_training=True):
    """Mean softmax cross entropy with label smoothing (imagenet_train_eval.py:578-584); the l2 term's gradient is
    applied by the fused update kernel."""
    return gnn.softmax_cross_entropy(self(images, is_training), labels, label_smoothing)

  def infer(self, images):
    """Eval forward: the training forward's kernels without autograd (there is no batch norm to freeze) -> fp32 logits."""
    self._check_input(images)
    with torch.no_grad():
      self.graph.refresh_shadows()
      x, prev = images.contiguous(), 1
      for conv, st in self.convs:
        if st != prev:
          x, _ = ops.maxpool_fwd(self._pool_desc(x), x)
          prev = st
        n, h, w, _ = x.shape
        x = ops.conv_fwd_relu(conv.desc_for(n, h, w), x, conv.vars.ohwi)
      pooled = ops.global_avgpool_fwd(x)
      if self.fc_dense:
        return gnn.dense_infer(self.fc, pooled).float()
      n = pooled.shape[0]
      return ops.conv_fwd(self.fc.desc_for(n, 1, 1), pooled.reshape(n, 1, 1, -1), self.fc.vars.ohwi).reshape(n, -1).float()


def synthetic_batch(batch, device, seed=1234, image_size=224, num_classes=1000):
  gen = torch.Generator(device=device).manual_seed(seed)
  images = torch.randn(batch, image_size, image_size, 3, generator=gen, device=device).to(torch.bfloat16)
  labels = torch.randint(0, num_classes, (batch,), generator=gen, device=device)
  return images, labels
