"""Inner optimizers with the tf.train.Optimizer surface the reference wraps
(``compute_gradients`` / ``apply_gradients`` / ``minimize`` / slots), executing
on the fused HIP update kernels (K3, rigl_masked_sgd_momentum / rigl_masked_adam).

  tf.train.MomentumOptimizer(lr, momentum, use_nesterov=True)
      rigl/imagenet_resnet/imagenet_train_eval.py:360-361,
      rigl/cifar_resnet/resnet_train_eval.py:202-203, mnist_train_eval.py:263
  tf.train.GradientDescentOptimizer(lr)      rigl/sparse_optimizers_test.py:44
  tf.train.AdamOptimizer(lr)                 imagenet_train_eval.py:355-358 (--use_adam),
      mnist_train_eval.py:247-261 (--optimizer=adam)

Eager twin of the TF1 graph API: ``compute_gradients(loss)`` runs the backward
pass (the masked-layer autograd bridge deposits DENSE kernel gradients in the
gradient arena); ``apply_gradients`` enqueues one update launch per arena
segment:  masked kernels (bitmap, weight decay) | dense kernels | BN & biases.
The l2 regulariser's gradient (scale * w on the raw variable) is
applied inside the kernel rather than through the loss.

``learning_rate``: a float, a callable ``lr(global_step) -> float`` evaluated on the host every step (both reach the
kernels by value), or a ``schedules.Schedule``.  On a GPU graph a Schedule takes the DEVICE path: the step counter and
the rate live in device memory, one ``ops.lr_schedule_step`` per apply evaluates the schedule there, and the update
kernels read the rate through a pointer -- so ``GraphedStep`` replays one graph through the whole schedule (the
counter is kept by the protocol of ``step_state``).
"""
import torch

from rigl_amd import _lib
from rigl_amd import ops
from rigl_amd import schedules
from rigl_amd import variables as V
from rigl_amd.step_state import StepCounter


def get_or_create_global_step(graph=None):
  return (graph or V.get_default_graph()).get_or_create_global_step()


def _lr_value(lr, global_step):
  if callable(lr):
    return float(lr(int(global_step.value) if global_step is not None else 0))
  return float(lr)


def inner_optimizer(optimizer):
  """The optimizer of this module behind ``optimizer``: itself, or what a sparse wrapper holds as ``_optimizer``."""
  return getattr(optimizer, '_optimizer', optimizer)


def _gpu_scalar(t):
  return torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.numel() == 1


class _DeviceLr:
  """The device path of a schedules.Schedule: its step ``counter`` and the fp32 [1] ``rate`` the update kernels read.
  ``step`` enqueues this step's rate: *rate = schedule(*counter); *counter += 1."""

  def __init__(self, device):
    self.counter = StepCounter(device, 'learning-rate')
    self.rate = torch.zeros(1, dtype=torch.float32, device=device)

  def step(self, schedule, global_step):
    self.counter.sync(global_step)
    ops.lr_schedule_step(schedule.descriptor(), self.counter.tensor, self.rate)
    self.counter.moved(1)


class Optimizer:
  """Minimal tf.train.Optimizer base."""

  def __init__(self, use_locking=False, name='Optimizer', graph=None):
    self._use_locking = use_locking
    self._name = name
    self._graph = graph

  @property
  def graph(self):
    return self._graph or V.get_default_graph()

  def get_slot_names(self):
    return []

  def get_slot(self, var, name):
    raise KeyError(name)

  def minimize(self, loss, global_step=None, var_list=None, **kwargs):
    grads_and_vars = self.compute_gradients(loss, var_list=var_list, **kwargs) \
        if var_list is not None else self.compute_gradients(loss, **kwargs)
    return self.apply_gradients(grads_and_vars, global_step=global_step)


class GradientDescentOptimizer(Optimizer):
  """w -= lr * g  (g = mask * dense_grad + wd * w for masked kernels)."""

  def __init__(self, learning_rate, use_locking=False,
               name='GradientDescent', graph=None, grad_sync=None):
    super().__init__(use_locking, name, graph)
    self._lr = learning_rate
    self._momentum = None
    self._nesterov = False
    self._slot = None              # flat momentum arena (same layout as W)
    self._grad_sync = grad_sync    # rigl_amd.dist.GradSync or None
    self._backward_done_for = None
    self.dense_masked_update = False   # DNW: apply the dense gradient to masked kernels too
    # the _DeviceLr of a schedules.Schedule on a GPU graph.  Created by the first apply, an eager one (GraphedStep runs eager
    # steps before it captures), so its buffers never belong to a graph-private pool
    self.device_lr = None
    # summaries.TrainingSummaries.attach() sets it: called once per apply, in front of the first update launch.  None: no launch
    self.summary_hook = None
    # the MicroBatches whose sum is pending or finished for the loss being minimised (set by its call), or None
    self.accumulation = None

  # ---- gradients -------------------------------------------------------------
  def compute_gradients(self, loss, var_list=None, **kwargs):
    """Returns [(grad, var)].  With ``var_list`` = the masked weights (RigL's
    second call, sparse_optimizers_base.py:481-482) the DENSE gradients are
    returned -- they are a by-product of the same backward pass."""
    del kwargs
    g = self.graph
    g.finalize()
    acc = self.accumulation
    if acc is not None and loss is not None:
      acc.check_pending(loss)      # a sum pending for another loss: refused, never guessed
    if loss is not None and self._backward_done_for is not loss:
      g.zero_other_grads()
      # a sum pending for this loss under a gradient exchange: the LAST pass runs range by range in front of each collective
      exchanged = acc is not None and acc.arm_exchange(loss)
      try:
        loss.backward()
        self._backward_done_for = loss
        if acc is not None and not exchanged:
          acc.finish(loss)         # the LAST pass of a pending sum: the arena holds the raw sum before anything reads it
        if self._grad_sync is not None:
          self._grad_sync.all_reduce(g)
      finally:
        if exchanged:
          acc.disarm_exchange()
    if var_list is not None:
      return [(v.grad, v) for v in var_list]
    # (the list handed out is remembered: getting it back untouched needs no per-variable check in apply_gradients)
    self._last_gv = [(v.grad, v) for v in g.trainable_variables()]
    return self._last_gv

  # ---- update ----------------------------------------------------------------
  def update_scale(self):
    """The factor the update kernels (momentum and Adam alike) and the summaries apply to the arena's gradient: the 1 / world
    of a GradSync, whose all-reduce leaves the sum over replicas, times the 1 / k of a MicroBatches accumulation finished for
    the loss that was backpropagated, which leaves the sum over micro-batches."""
    scale = self._grad_sync.grad_scale if self._grad_sync is not None else 1.0
    acc = self.accumulation
    if acc is not None and acc.finished_for(self._backward_done_for):
      scale = scale * acc.inv_k
    return scale

  def forget_backward(self):
    """The last backward no longer counts: the next compute_gradients backpropagates its loss, whichever it is."""
    self._backward_done_for = None

  def step_loss(self):
    """The loss of the step being applied, for its record: the micro-batch mean when a MicroBatches covers the loss that was
    backpropagated, otherwise that loss; detached, or None where it is not one fp32 scalar on the GPU."""
    loss, acc = self._backward_done_for, self.accumulation
    if acc is not None and acc.finished_for(loss):
      loss = acc.loss
    return loss.detach() if _gpu_scalar(loss) else None

  def _ensure_slots(self):
    """Creates the slot arenas (plain gradient descent has none)."""

  def lr_on_device(self):
    """True when the learning rate is a schedules.Schedule and the graph lives on a GPU: the rate is then computed and
    read on the device (see the module docstring).  ``Schedule.host_only()`` forces the host path."""
    w = self.graph.W
    return isinstance(self._lr, schedules.Schedule) and w is not None and w.is_cuda

  def lr_key(self, global_step):
    """What a captured graph of this optimizer's step holds of the rate: the Schedule itself on the device path (the graph
    evaluates it), otherwise the rate's value at ``global_step`` (a kernel argument, frozen at capture)."""
    return self._lr if self.lr_on_device() else _lr_value(self._lr, global_step)

  def step_participants(self):
    """The step_state participants of the next apply, each with ``fresh(global_step)`` and ``moved(k)``: the device rate's
    counter on the device path (None until the first eager apply has allocated it) and the attached summaries."""
    parts = [self.summary_hook] if self.summary_hook is not None else []
    if self.lr_on_device():
      parts.append(self.device_lr.counter if self.device_lr is not None else None)
    return parts

  def apply_gradients(self, grads_and_vars, global_step=None, name=None):
    del name
    g = self.graph
    g.finalize()
    # The kernels read the gradient arena.  Gradients handed back unchanged ARE arena slices; transformed ones
    # (clipping, scaling) are copied into their variable's slice; what the arena-wide update cannot express --
    # a None gradient or a subset of the trainable variables -- raises instead of being silently ignored.
    if grads_and_vars is not None and grads_and_vars is not getattr(self, '_last_gv', None):
      gv = list(grads_and_vars)
      seen = set()
      for grad, var in gv:
        if grad is None:
          raise NotImplementedError('apply_gradients: None gradient for %s (the fused update walks whole arena '
                                    'segments; freeze a variable by zeroing its gradient instead)' % var.name)
        if not hasattr(var, 'grad') or var.grad is None:
          raise ValueError('apply_gradients: %r is not a variable of this graph' % (var,))
        if grad.data_ptr() != var.grad.data_ptr():
          var.grad.copy_(grad.reshape(var.grad.shape))
        seen.add(var.name)
      missing = [v.name for v in g.trainable_variables() if v.name not in seen]
      if gv and missing:
        raise NotImplementedError('apply_gradients: the fused update covers every trainable variable; missing %s%s'
                                  % (missing[:3], ' ...' if len(missing) > 3 else ''))
    self._ensure_slots()
    if self.lr_on_device():
      if self.device_lr is None:
        self.device_lr = _DeviceLr(g.W.device)
      self.device_lr.step(self._lr, global_step)
      lr = self.device_lr.rate       # the update launches read it on the device
    else:
      lr = _lr_value(self._lr, global_step)
    scale = self.update_scale()
    mu = float(self._momentum) if self._momentum is not None else 0.0
    if self.summary_hook is not None:
      # this step's record: the weights and gradients as they are now
      self.summary_hook.on_apply(global_step, self.step_loss(), lr, scale)
    # one launch per segment; weight decay is uniform inside a kernel segment
    for kind in (V.KIND_MASKED, V.KIND_DENSE):
      b, e = g.seg[kind]
      if e <= b:
        continue
      wds = {v.weight_decay for v in g.trainable_variables() if v.kind == kind}
      if len(wds) > 1:
        self._apply_per_variable(kind, lr, mu, scale)
        continue
      wd = wds.pop() if wds else 0.0
      if kind == V.KIND_MASKED and self.dense_masked_update:
        wd = 0.0                 # DNW: gradients are taken w.r.t. mask*W, which the l2 regulariser does not reach
      self._apply_range(b, e, (g.BITS[b // 32:e // 32]
                               if kind == V.KIND_MASKED and not self.dense_masked_update else None),
                        lr, mu, wd, scale)
    b, e = g.seg[V.KIND_OTHER]
    if e > b:
      self._apply_range(b, e, None, lr, mu, 0.0, scale)
    self._finish()
    g.shadows_dirty = True
    self.forget_backward()
    if self.accumulation is not None:
      self.accumulation.release()
    if global_step is not None:
      global_step.value += 1
    return None

  def _apply_per_variable(self, kind, lr, mu, scale):
    g = self.graph
    for l in g.layers:
      v = l.weights
      if v.kind != kind:
        continue
      o, n = v.offset, v.numel
      n4 = (n + 3) // 4 * 4  # padding inside the 64-aligned slot is harmless
      self._apply_range(o, o + n4, (l.mask.bits if l.mask is not None and not self.dense_masked_update else None),
                        lr, mu, (0.0 if (kind == V.KIND_MASKED and self.dense_masked_update) else v.weight_decay),
                        scale)

  def _apply_range(self, b, e, mask_bits, lr, mu, wd, scale):
    """One update launch over arena elements [b, e) (K3).  ``lr``: a float, or the device rate's tensor."""
    g = self.graph
    ops.masked_sgd_momentum(
        g.W[b:e], g.G[b:e], momentum=self._slot[b:e] if self._slot is not None else None,
        mask_bits=mask_bits, mu=mu, weight_decay=wd, grad_scale=scale, nesterov=self._nesterov, **ops.lr_kwargs(lr))

  def _finish(self):
    """After the last segment of a step (tf.train.Optimizer._finish)."""


class MomentumOptimizer(GradientDescentOptimizer):
  """TF ApplyMomentum: accum = accum*momentum + g;
  w -= lr*g + lr*momentum*accum (use_nesterov) | w -= lr*accum."""

  def __init__(self, learning_rate, momentum, use_locking=False,
               name='Momentum', use_nesterov=False, graph=None, grad_sync=None):
    super().__init__(learning_rate, use_locking, name, graph, grad_sync)
    self._momentum = momentum
    self._nesterov = use_nesterov

  def get_slot_names(self):
    return ['momentum']

  def _ensure_slots(self):
    g = self.graph
    if self._slot is None or self._slot.numel() != g.W.numel():
      old = self._slot
      self._slot = torch.zeros_like(g.W)
      if old is not None:
        raise RuntimeError('variables were added after the momentum slots '
                           'were created')

  def get_slot(self, var, name):
    if name != 'momentum':
      raise KeyError(name)
    self.graph.finalize()
    self._ensure_slots()
    return self._slot[var.offset:var.offset + var.numel].view(var.shape)


class AdamOptimizer(GradientDescentOptimizer):
  """tf.train.AdamOptimizer (TF ApplyAdam, non-Nesterov) on K3-Adam (rigl_masked_adam):
    alpha = (lr * sqrt(1 - beta2_power)) / (1 - beta1_power)
    m += (g - m) * (1 - beta1);  v += (g*g - v) * (1 - beta2);  w -= (m * alpha) / (sqrt(v) + epsilon)
  with g = mask * grad_scale * dense + wd * w as for the momentum path.  Masked-off weights are updated too (the
  reference applies Adam to the raw variable).  Slots 'm' and 'v' are two flat arenas with the layout of W; the
  beta powers are a device buffer (beta1_power, beta2_power) that starts at (beta1, beta2) and is multiplied by them
  once per apply_gradients, after every variable is updated (_finish) -- mask-update iterations of RigL do not call
  the inner apply and so do not advance it.  Used by imagenet_train_eval.py --use_adam (:214-215, 355-358) and
  mnist_train_eval.py --optimizer=adam (:247-261)."""

  def __init__(self, learning_rate=0.001, beta1=0.9, beta2=0.999, epsilon=1e-8, use_locking=False, name='Adam',
               graph=None, grad_sync=None):
    super().__init__(learning_rate, use_locking, name, graph, grad_sync)
    self._beta1 = float(beta1)
    self._beta2 = float(beta2)
    self._epsilon = float(epsilon)
    self._slot_v = None            # second flat arena ('v'); self._slot is 'm'
    self._beta_powers = None       # device fp32 [2]

  def get_slot_names(self):
    return ['m', 'v']              # TF sorts the slot names

  def _ensure_slots(self):
    g = self.graph
    if self._slot is None or self._slot.numel() != g.W.numel():
      if self._slot is not None:
        raise RuntimeError('variables were added after the Adam slots were created')
      self._slot = torch.zeros_like(g.W)
      self._slot_v = torch.zeros_like(g.W)
      self._beta_powers = torch.tensor([self._beta1, self._beta2], dtype=torch.float32, device=g.W.device)

  def get_slot(self, var, name):
    if name not in ('m', 'v'):
      raise KeyError(name)
    self.graph.finalize()
    self._ensure_slots()
    arena = self._slot if name == 'm' else self._slot_v
    return arena[var.offset:var.offset + var.numel].view(var.shape)

  def _get_beta_accumulators(self):
    """Host copies (beta1_power, beta2_power) of the device accumulators."""
    self.graph.finalize()
    self._ensure_slots()
    bp = self._beta_powers.cpu()
    return bp[0].item(), bp[1].item()

  def _apply_range(self, b, e, mask_bits, lr, mu, wd, scale):
    del mu
    g = self.graph
    ops.masked_adam(g.W[b:e], g.G[b:e], self._slot[b:e], self._slot_v[b:e], self._beta_powers, beta1=self._beta1,
                    beta2=self._beta2, epsilon=self._epsilon, mask_bits=mask_bits, weight_decay=wd, grad_scale=scale,
                    **ops.lr_kwargs(lr))

  def _finish(self):
    ops.adam_advance(self._beta_powers, self._beta1, self._beta2)


class MicroBatches:
  """k micro-batches, one optimizer step: a k-replica run of the reference (per-core batch, gradients summed over cores,
  imagenet_train_eval.py:363-365) serialised onto one GPU.

    mb = MicroBatches(loss_fn, optimizer, micro_batches=k)   # a callable with loss_fn's signature
    optimizer.minimize(mb(), gs)                             # eager
    step = GraphedStep(mb, optimizer, gs)                    # one captured graph = k passes + one update
    mb.loss                                                  # device fp32 [1]: mean of the step's k micro-batch losses

  ``optimizer``: an inner optimizer of this module or a wrapper around one (its ``_optimizer``).  ``mb()`` runs micro-batches
  1..k-1 itself -- loss_fn(), zero_other_grads(), backward(), one ops.grad_accumulate pass over the whole gradient arena (FIRST,
  then ADD) into a second arena -- calls loss_fn() a k-th time and returns THAT loss, with the sum pending against it.  The
  inner optimizer's compute_gradients backpropagates it as always and then enqueues the LAST pass, once and in front of every
  reader: the arena holds the raw fp32 SUM fl(fl(g1+g2)+g3)..., which is what RigL's grow scores, DNW, pruning and the
  summaries read (the reference's cross-replica sum, sparse_optimizers_base.py:472-473), and the mean is folded into the
  update's grad_scale (update_scale).  compute_gradients on another loss while a sum is pending raises.

  Once per call, i.e. per optimizer step: the global step, the learning-rate counter, the summaries record (its loss is
  ``mb.loss``), the mask-update schedule, weight decay and the Adam beta powers.  Once per micro-batch: batch-norm batch
  statistics and moving-average updates, dropout draws, DeviceCifar.next_batch() -- k consecutive forward passes, like k
  replicas.  A mask-update call runs its k micro-batches too and hands the mask update the raw sum.

  With k == 1 ``mb()`` is ``loss_fn()``: no pass is enqueued, no buffer is allocated, no scale changes.  Every launch goes
  into whatever is being captured and every buffer (the second arena, the loss accumulator and mean) is allocated here, so
  GraphedStep(mb, ...) captures and replays the k passes and the update as one graph.

  With data parallelism (the inner optimizer's ``grad_sync`` is an enabled dist.GradSync -- world > 1, or forced on with one rank)
  this is the reference's headline configuration, replicas x per-core batches (8 x 4 x 128 = 4096), with ONE gradient exchange
  per optimizer step.  Passes 1..k-1 hold the exchange: no collective is enqueued, each is followed by the whole-arena FIRST /
  ADD pass as above.  In the k-th backward pass every exchange bucket [lo, hi) that becomes ready first gets a LAST pass over
  exactly that range (ops.grad_accumulate_ranges, on the compute stream) and then its asynchronous all-reduce, so the exchange
  overlaps the k-th backward bucket by bucket like a plain data-parallel step's; the final flush behind backward is one LAST
  launch over the head of the kernel segment and the BN / bias segment, which carries the loss arithmetic, followed by the
  coalesced collective.  Every element of the arena gets LAST exactly once and the whole-arena LAST is not run.  The arena then
  holds the raw sum over ranks AND micro-batches -- fl(S_0 + S_1 + ...) of the ranks' sequential micro-batch sums S_r -- which
  the mask update, DNW, pruning and the summaries read; update_scale() is 1 / world x 1 / k, the one place either factor lives.
  ``mb.loss`` stays the RANK-LOCAL mean of this rank's k micro-batch losses (the reference logs the per-core loss, too); reduce
  it over ranks yourself where a global figure is wanted.  k == 1 with a GradSync enqueues exactly what a plain data-parallel
  step enqueues.  GraphedStep runs data-parallel steps eagerly, accumulated or not.  A GradSync that exchanges another graph's
  arena than the optimizer's is refused (NotImplementedError): its buckets would not be ranges of the arena summed here."""

  def __init__(self, loss_fn, optimizer, micro_batches):
    k = int(micro_batches)
    if k < 1 or k != micro_batches:
      raise ValueError('micro_batches must be an integer >= 1, got %r' % (micro_batches,))
    inner = inner_optimizer(optimizer)
    if not hasattr(inner, 'accumulation'):
      raise TypeError('%s cannot accumulate (expected a rigl_amd.train optimizer or a wrapper around one)' % type(inner).__name__)
    sync = getattr(inner, '_grad_sync', None)
    if sync is None or not getattr(sync, 'enabled', False):
      sync = None
    elif getattr(sync, 'graph', None) is not inner.graph:
      raise NotImplementedError('MicroBatches: the GradSync does not exchange the gradient arena of the optimizer\'s graph; '
                                'holding and finishing the exchange of another arena is not supported')
    self._sync = sync              # the enabled GradSync whose exchange is held back to the k-th pass, or None
    self._loss_fn = loss_fn
    self._inner = inner
    self.micro_batches = k
    self.inv_k = 1.0 / k
    self._pending = None           # the k-th loss, between __call__ and the compute_gradients that backpropagates it
    self._done_for = None          # the loss whose LAST pass was enqueued: the arena holds its sum
    self._last = None              # k == 1: the loss of the last call
    self._arena = self._loss_acc = self._loss_mean = None
    if k > 1:
      g = inner.graph
      g.finalize()
      if g.W is None or not g.W.is_cuda:
        raise _lib.RiglError(_lib.RIGL_EINVAL, 'MicroBatches needs a graph on the GPU (no CPU path exists)')
      self._build()
      g.add_relayout_callback(self._build)

  def _build(self):
    """(Re)allocates the second arena with the layout of G, and the two loss scalars."""
    G = self._inner.graph.G
    self._arena = torch.empty_like(G)       # FIRST overwrites all of it: never read before it is written
    self._loss_acc = torch.zeros(1, dtype=torch.float32, device=G.device)
    self._loss_mean = torch.zeros(1, dtype=torch.float32, device=G.device)
    self._pending = self._done_for = None

  @property
  def loss(self):
    """Device fp32 [1]: the mean of the k micro-batch losses of the last step whose gradients were computed."""
    if self.micro_batches == 1:
      return None if self._last is None else self._last.reshape(1)
    return self._loss_mean

  @staticmethod
  def _check_loss(loss):
    if not _gpu_scalar(loss):
      raise TypeError('MicroBatches: loss_fn must return one fp32 scalar on the GPU')
    return loss.detach()

  def __call__(self, *args, **kwargs):
    if self.micro_batches == 1:
      loss = self._loss_fn(*args, **kwargs)
      self._last = loss.detach() if torch.is_tensor(loss) else None   # (an alias of the value, not of the autograd graph)
      return loss
    inner = self._inner
    g = inner.graph
    g.finalize()
    # A new step begins: nothing of the last one is kept.  A loss tensor that stays referenced keeps its autograd graph's
    # AccumulateGrad nodes of the bias / batch-norm leaves alive, the next forward pass reuses them, and they run on the
    # stream they were created on -- for ever the stream of the first step.  A step captured on another stream would pull
    # that stream into its capture.  So the references taken here live from this call to the apply (or the next call).
    self._pending = self._done_for = None
    inner.forget_backward()
    sync = self._sync
    if sync is not None:
      sync.held = True             # these passes' gradients are partial sums: nothing is exchanged, no bucket state is kept
    try:
      for i in range(self.micro_batches - 1):
        loss = self._loss_fn(*args, **kwargs)
        scalar = self._check_loss(loss)
        g.zero_other_grads()
        loss.backward()
        ops.grad_accumulate(self._arena, g.G, _lib.ACC_FIRST if i == 0 else _lib.ACC_ADD,
                            loss=scalar, loss_acc=self._loss_acc)
        del loss, scalar
    finally:
      if sync is not None:
        sync.held = False
    loss = self._loss_fn(*args, **kwargs)
    self._check_loss(loss)
    self._pending = loss
    inner.accumulation = self
    return loss

  # ---- the inner optimizer's side ------------------------------------------------------------------------------------------
  def check_pending(self, loss):
    if self._pending is not None and self._pending is not loss:
      raise RuntimeError('compute_gradients on another loss while the sum of %d micro-batches is pending: pass the tensor '
                         'MicroBatches.__call__ returned' % (self.micro_batches - 1))

  def finish(self, loss):
    """Behind the backward pass of ``loss``: the LAST pass, when the sum is pending for exactly this tensor."""
    if self._pending is None or self._pending is not loss:
      return
    ops.grad_accumulate(self._arena, self._inner.graph.G, _lib.ACC_LAST, loss=loss.detach(),
                        loss_acc=self._loss_acc, loss_mean=self._loss_mean, inv_k=self.inv_k)
    self._pending, self._done_for = None, loss

  def arm_exchange(self, loss):
    """In front of the backward pass of ``loss``: with a gradient exchange and the sum pending for exactly this tensor, the
    LAST pass is handed to the exchange (True) -- range by range in front of each collective -- and finish() is not to run."""
    if self._sync is None or self._pending is None or self._pending is not loss:
      return False
    self._sync.before_exchange = self._last_ranges
    return True

  def disarm_exchange(self):
    self._sync.before_exchange = None

  def _last_ranges(self, ranges, final):
    """GradSync.before_exchange: the LAST pass over the arena ranges [(lo, hi)] about to be sent; the flush behind backward
    (``final``) carries the loss arithmetic and ends the pending sum."""
    spans = [(lo, hi - lo) for lo, hi in ranges]
    G = self._inner.graph.G
    if not final:
      ops.grad_accumulate_ranges(self._arena, G, spans, _lib.ACC_LAST)
      return
    loss = self._pending
    ops.grad_accumulate_ranges(self._arena, G, spans, _lib.ACC_LAST, loss=loss.detach(), loss_acc=self._loss_acc,
                               loss_mean=self._loss_mean, inv_k=self.inv_k)
    self._pending, self._done_for = None, loss

  def finished_for(self, loss):
    return loss is not None and self._done_for is loss

  def release(self):
    """The update was applied: the step's loss is let go of (see __call__)."""
    self._done_for = None


class GraphedStep:
  """One training step replayed from a captured HIP graph (torch.cuda.CUDAGraph over the kernels the
  C ABI enqueues on the current stream) -- for launch-bound models, where the ~250 launches of a step cost
  more on the host than on the device (CIFAR WRN-22 at batch 128: 2.4 ms eager, the device work is a
  fraction of that).  ResNet-50 at batch 128 is device-bound and gains < 1 % (tools/graph_probe.py), so the
  headline benchmark stays eager.

  Only ORDINARY iterations are replayed: the schedule (``is_mask_update_iter``) is host arithmetic on the
  global step, so it is evaluated before every call and mask-update iterations (one in ``frequency``) run
  eagerly -- they change the masks the captured kernels read through the same buffers, which is fine: the
  graph holds pointers, not values.  Scalars that are kernel ARGUMENTS are frozen at capture: the gradient
  scale, and a learning rate given as a float or a plain callable (a new graph is captured whenever
  ``lr(global_step)`` changes: piecewise-constant schedules recapture a handful of times; while the value
  changes every step -- a warm-up, a cosine -- nothing is captured and the steps run eagerly).  A learning rate
  given as a ``schedules.Schedule`` is NOT frozen: the optimizer keeps the step counter and the rate in device
  memory and the captured step itself evaluates the schedule and advances the counter (ops.lr_schedule_step), so
  ONE graph, keyed on the schedule object, is replayed through warm-up, drops and restarts alike.  That counter
  and whatever else the optimizer names (``step_participants``) is kept by the protocol of ``step_state``: a call that finds
  one stale runs eagerly -- a graph is never replayed against a stale counter.  The loss tensor is the captured step's output.

  ``loss_fn`` must read its inputs from fixed device buffers (copy each new batch into them); a ``MicroBatches`` as ``loss_fn``
  puts its k forward / backward passes and the one update into the same graph.  Data-parallel
  steps (a GradSync with world > 1) are not captured -- the collectives stay eager -- and run as usual.
  """

  def __init__(self, loss_fn, optimizer, global_step, warmup=3):
    self._loss_fn = loss_fn
    self._opt = optimizer
    self._gs = global_step
    self._warmup = warmup
    self._graphs = {}          # lr value (or the Schedule object on the device path) -> (CUDAGraph, loss tensor)
    self._inner = inner_optimizer(optimizer)
    sync = getattr(self._inner, '_grad_sync', None)
    self._eager_only = (sync is not None and getattr(sync, 'enabled', False)) or not torch.cuda.is_available()
    self.replays = 0
    self.eager_steps = 0
    self._ws_gen = ops.WORKSPACE_GENERATION
    self._last_key = None      # learning-rate key of the previous ordinary step: the second consecutive one at a rate captures
    self._parts = None         # the step_state participants the cached graphs were captured with

  def _is_update(self):
    o = self._opt
    if not hasattr(o, 'is_mask_update_iter'):
      return False
    return bool(o.is_mask_update_iter(int(self._gs.value), o._last_update_step))   # pylint: disable=protected-access

  def _eager(self):
    loss = self._loss_fn()
    self._opt.minimize(loss, self._gs)
    self.eager_steps += 1
    return loss

  def __call__(self):
    if self._eager_only or self._is_update():
      return self._eager()
    parts = self._inner.step_participants()
    if parts != self._parts:       # graphs captured with other participants (another hook, or none) enqueue another set of launches
      self._graphs.clear()
      self._parts = parts
    if any(p is None or not p.fresh(self._gs) for p in parts):
      return self._eager()         # allocates / uploads the stale device counter (never in a graph)
    if self._ws_gen != ops.WORKSPACE_GENERATION:
      # a scratch buffer was (re)allocated since the graphs were captured (an eager mask update outgrew one, typically):
      # EVERY cached graph may point at the old buffer -- drop them all and capture again.  Checked before every replay,
      # so no graph is ever replayed against a freed buffer (ops.workspace keeps nothing alive for them).
      self._graphs.clear()
      self._ws_gen = ops.WORKSPACE_GENERATION
    key = self._inner.lr_key(self._gs)
    if key in self._graphs:
      self._last_key = key
      return self._replay(key, parts)
    #  a learning rate that changes every step (linear warm-up, cosine) never reuses a graph keyed on its
    # value: while the key keeps changing, run plain eager steps and do not capture; at the second consecutive step with
    # the same key (the constant plateaus of a piecewise schedule), capture again.
    if not self._inner.lr_on_device():   # (the device path has one key for the whole schedule)
      stable, self._last_key = key == self._last_key, key
      if not stable:
        return self._eager()
    if self._warmup > 0:           # allocator / workspace caches / descriptors settle first
      self._warmup -= 1
      return self._eager()
    return self._capture(key, parts)

  def _capture(self, key, parts):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
      out = self._eager()          # THIS call's step, on a side stream as torch's capture recipe asks
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    if self._is_update() or self._inner.lr_key(self._gs) != key:
      return out                   # the next iteration is not an ordinary one at this lr: capture later
    gen0 = ops.WORKSPACE_GENERATION
    step1 = self._gs.value
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
      loss = self._loss_fn()
      self._opt.minimize(loss, self._gs)
    self._gs.value = step1         # capture enqueues nothing; undo its host side effect
    for p in parts:
      p.moved(-1)
    if gen0 != ops.WORKSPACE_GENERATION or gen0 != self._ws_gen:
      # a buffer grew during the pre-capture step or the capture itself: graphs cached under other learning rates are
      # stale, and this one may hold both addresses -- keep none, the next call captures on settled buffers
      self._graphs.clear()
      self._ws_gen = ops.WORKSPACE_GENERATION
      return out
    if len(self._graphs) >= 16:
      self._graphs.pop(next(iter(self._graphs)))   # bound the cache (piecewise-constant schedules have few values)
    self._graphs[key] = (graph, loss)
    return out

  def _replay(self, key, parts):
    graph, loss = self._graphs[key]
    graph.replay()
    self._gs.value += 1
    for p in parts:
      p.moved(1)                   # (the summaries: the replay wrote this step's record)
    self._inner.graph.shadows_dirty = True   # the replayed update rewrote the weights
    self.replays += 1
    return loss
