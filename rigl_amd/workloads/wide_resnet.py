"""CIFAR WideResNet (pre-activation, depth = 6n+4) from the masked layers --
rigl/cifar_resnet/resnet_model.py:70-235.  BASELINE config 2 ("CIFAR-10
ResNet-20") is depth 22, width 1.

Kept from the reference: every 3x3 conv uses TF 'SAME' even at stride 2
(asymmetric (0,1) padding on 32->16 and 16->8); the 1x1 skip conv is 'VALID'
with the block's stride and takes the pre-activated tensor; the stem is dense
unless ``prune_first_layer``; final BN-ReLU -> avg-pool 8 -> masked logits;
l2 5e-4 on kernels; Dropout(droprate) between bn_b's ReLU and conv2 while training
(resnet_model.py:224-231), off (``droprate=0.0``) unless asked for.
"""
import torch

from rigl_amd import pruning_layers as PL
from rigl_amd import pyhash
from rigl_amd import variables as V
from rigl_amd.workloads import nn as gnn
from rigl_amd.workloads import shapes as WS


class WideResNet:

  def __init__(self, graph=None, depth=22, width=1, num_classes=10,
               pruning_method='threshold', prune_first_layer=False,
               prune_last_layer=True, weight_decay=5e-4, seed=0, droprate=0.0, dropout_seed=0):
    """``droprate``: the reference's constructor default is 0.3 (resnet_model.py:41); here the default is 0.0 (no dropout,
    no extra launch) so that parity and benchmark runs stay deterministic.  With ``droprate`` in (0, 1) every training
    forward advances ``dropout_state.step`` (device int32) and drops after bn_b's ReLU with the keep mask of
    tf.random.stateless_uniform(seed=[dropout_seed0(block), step]); ``infer`` and ``is_training=False`` are unchanged.
    Data-parallel callers pass a rank-distinct ``dropout_seed`` (every rank would otherwise drop the same positions)."""
    if not 0.0 <= droprate < 1.0:
      raise ValueError('droprate must be in [0, 1), got %r' % (droprate,))
    self.graph = g = graph or V.get_default_graph()
    self.droprate, self.dropout_seed = float(droprate), int(dropout_seed)
    self.dropout_state = gnn.DropoutState(g.device) if self.droprate > 0 else None
    PL.set_init_seed(seed)
    tech = pruning_method

    def conv(name, k, cin, cout, stride, padding, technique, need_dx=True):
      scope = WS.SCOPE + '/' + name
      layer = PL.MaskedConv2d(g, scope, cin, cout, (k, k), (stride, stride), padding, technique, weight_decay,
                              PL.variance_scaling_initializer(), need_dx)
      g.modules[scope] = layer
      return layer

    self.stem = conv('conv_1', 3, 3, 16, 1, 'SAME', tech if prune_first_layer else 'baseline', need_dx=False)
    self.blocks = []
    cur = None
    for name, k, cin, cout, stride, kind in WS.wide_resnet_convs(depth, width):
      if kind == 'skip':
        cur = dict(skip=conv(name, 1, cin, cout, stride, 'VALID', tech))
      elif kind == 'conv1':
        cur = cur if (cur is not None and 'conv1' not in cur) else {}
        cur['bn_a'] = gnn.BatchNorm(g, '%s/%s_bn_a' % (WS.SCOPE, name), cin)
        cur['conv1'] = conv(name, 3, cin, cout, stride, 'SAME', tech)
        cur['bn_b'] = gnn.BatchNorm(g, '%s/%s_bn_b' % (WS.SCOPE, name), cout)
      else:
        cur['conv2'] = conv(name, 3, cout, cout, 1, 'SAME', tech)
        self.blocks.append(cur)
        cur = None
    self.final_bn = gnn.BatchNorm(g, WS.SCOPE + '/final_bn', 64 * width)
    self.logits = PL.MaskedDense(g, WS.SCOPE + '/logits', 64 * width, num_classes, True,
                                 tech if prune_last_layer else 'baseline', weight_decay)
    g.modules[WS.SCOPE + '/logits'] = self.logits
    g.finalize()
    self._dropout_seed0 = [self.dropout_seed0(i) for i in range(len(self.blocks))]

  def dropout_seed0(self, block_index):
    """seed0 of a block's dropout: int32(dropout_seed + hash(conv1 scope + '/dropout')), the convention of the mask update's
    seeds (sparse_optimizers._stable_hash: the builtin hash under a fixed PYTHONHASHSEED, else its PYTHONHASHSEED=0 value)."""
    v = self.dropout_seed + pyhash.name_hash(self.blocks[block_index]['conv1'].scope + '/dropout')
    return (v + (1 << 31)) % (1 << 32) - (1 << 31)

  def __call__(self, images, is_training=True):
    drop = bool(is_training and self.droprate > 0)
    if drop:
      from rigl_amd import ops  # pylint: disable=import-outside-toplevel
      ops.dropout_advance(self.dropout_state.step)   # on the device and inside whatever is captured: every replay draws fresh masks
    net = self.stem(images)
    for i, b in enumerate(self.blocks):
      skip = net
      net = b['bn_a'](net, is_training, relu=True)
      if 'skip' in b:
        skip = b['skip'](net)
      net = b['conv1'](net, bn_stats=True)          # its output goes straight into bn_b: statistics from the conv epilogue
      net = b['bn_b'](net, is_training, relu=True)
      if drop:
        net = gnn.dropout(net, self.droprate, self._dropout_seed0[i], self.dropout_state)   # (a fresh tensor: no hand-over attributes for conv2)
      net = b['conv2'](net)
      net = net + skip
    net = self.final_bn(net, is_training, relu=True)
    net = gnn.global_avg_pool(net)            # 8x8 map, pool_size 8
    return self.logits(net)

  def infer(self, images):
    """Eval forward (frozen batch norms; pre-activation: rigl_bn_apply, then the conv).  fp32 logits, no autograd."""
    from rigl_amd import ops  # pylint: disable=import-outside-toplevel
    with torch.no_grad():
      self.graph.refresh_shadows()
      p = gnn.infer_params(self.graph)
      net = gnn.conv_infer(self.stem, images)
      for b in self.blocks:
        skip = net
        net = ops.bn_apply(net, p[b['bn_a']], relu=True)
        if 'skip' in b:
          skip = gnn.conv_infer(b['skip'], net)
        net = ops.bn_apply(gnn.conv_infer(b['conv1'], net), p[b['bn_b']], relu=True)
        net = gnn.conv_infer(b['conv2'], net)
        net = net + skip
      net = ops.bn_apply(net, p[self.final_bn], relu=True)
      return gnn.dense_infer(self.logits, ops.global_avgpool_fwd(net)).float()

  def loss(self, images, labels, is_training=True):
    return gnn.softmax_cross_entropy(self(images, is_training), labels, 0.0)


def synthetic_batch(batch, device, seed=1234, num_classes=10, precision=None):
  gen = torch.Generator(device=device).manual_seed(seed)
  images = torch.randn(batch, 32, 32, 3, generator=gen, device=device).to(gnn.activation_dtype(precision))
  labels = torch.randint(0, num_classes, (batch,), generator=gen, device=device)
  return images, labels
