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
kernels read the rate through a pointer -- so ``GraphedStep`` replays one graph through the whole schedule.
"""
import torch

from rigl_amd import _lib
from rigl_amd import ops
from rigl_amd import schedules
from rigl_amd import variables as V


def get_or_create_global_step(graph=None):
  return (graph or V.get_default_graph()).get_or_create_global_step()


def _lr_value(lr, global_step):
  if callable(lr):
    return float(lr(int(global_step.value) if global_step is not None else 0))
  return float(lr)


def _int32(v):
  """v as the device's int32 counter holds it (two's-complement wrap-around)."""
  return (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31


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
    # the device path of a schedules.Schedule: int32 [1] step counter, fp32 [1] rate, and what the counter holds (host mirror)
    self._lr_step = None
    self._lr_dev = None
    self._lr_mirror = 0
    # summaries.TrainingSummaries.attach() sets it: called once per apply, in front of the first update launch.  None: no launch
    self._summary_hook = None
    # the MicroBatches whose sum is pending or finished for the loss being minimised (set by its call), or None
    self._accum = None

  # ---- gradients -------------------------------------------------------------
  def compute_gradients(self, loss, var_list=None, **kwargs):
    """Returns [(grad, var)].  With ``var_list`` = the masked weights (RigL's
    second call, sparse_optimizers_base.py:481-482) the DENSE gradients are
    returned -- they are a by-product of the same backward pass."""
    del kwargs
    g = self.graph
    g.finalize()
    acc = self._accum
    if acc is not None and loss is not None:
      acc.check_pending(loss)      # a sum pending for another loss: refused, never guessed
    if loss is not None and self._backward_done_for is not loss:
      g.zero_other_grads()
      loss.backward()
      self._backward_done_for = loss
      if acc is not None:
        acc.finish(loss)           # the LAST pass of a pending sum: the arena holds the raw sum before anything reads it
      if self._grad_sync is not None:
        self._grad_sync.all_reduce(g)
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
    acc = self._accum
    if acc is not None and acc.finished_for(self._backward_done_for):
      scale = scale * acc.inv_k
    return scale

  def _ensure_slots(self):
    self._ensure_lr_buffers()

  def lr_on_device(self):
    """True when the learning rate is a schedules.Schedule and the graph lives on a GPU: the rate is then computed and
    read on the device (see the module docstring).  ``Schedule.host_only()`` forces the host path."""
    w = self.graph.W
    return isinstance(self._lr, schedules.Schedule) and w is not None and w.is_cuda

  def _ensure_lr_buffers(self):
    """The persistent step / rate buffers of the device path.  First reached in an eager step (GraphedStep runs eager steps
    before it captures), so they never belong to a graph-private pool."""
    if self._lr_step is None and self.lr_on_device():
      dev = self.graph.W.device
      self._lr_step = torch.zeros(1, dtype=torch.int32, device=dev)
      self._lr_dev = torch.zeros(1, dtype=torch.float32, device=dev)
      self._lr_mirror = 0

  def _advance_lr_mirror(self, k):
    """The device counter moved by ``k`` without this optimizer's doing (a graph replay: +1; undoing a capture's host side
    effect: -1)."""
    self._lr_mirror = _int32(self._lr_mirror + k)

  def _device_lr_step(self, global_step):
    """Enqueues this step's rate: *lr = schedule(*step); *step += 1.  Invariant: before it, the device counter equals
    global_step.value (with global_step None it free-runs from 0).  Where the host mirror of the counter says otherwise --
    after global_step.assign, a checkpoint restore, a wrapper that stepped it some other way -- the counter is uploaded
    first; never during stream capture, where the upload would be replayed with its frozen value."""
    if global_step is not None:
      want = _int32(global_step.value)
      if want != self._lr_mirror:
        if torch.cuda.is_current_stream_capturing():
          raise RuntimeError('the device step counter (%d) differs from global_step (%d) during graph capture: run one eager '
                             'step after changing global_step' % (self._lr_mirror, want))
        self._lr_step.fill_(want)
        self._lr_mirror = want
    ops.lr_schedule_step(self._lr.descriptor(), self._lr_step, self._lr_dev)
    self._advance_lr_mirror(1)

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
      self._device_lr_step(global_step)
      lr = None                      # the update launches read self._lr_dev
    else:
      lr = _lr_value(self._lr, global_step)
    scale = self.update_scale()
    mu = float(self._momentum) if self._momentum is not None else 0.0
    if self._summary_hook is not None:
      self._summary_hook.on_apply(self, global_step, lr, scale)    # this step's record: the weights and gradients as they are now
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
    self._backward_done_for = None
    if self._accum is not None:
      self._accum.release()
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
    """One update launch over arena elements [b, e) (K3).  ``lr`` None: the rate is read from the device buffer."""
    g = self.graph
    ops.masked_sgd_momentum(
        g.W[b:e], g.G[b:e], lr, lr_device=self._lr_dev if lr is None else None,
        momentum=self._slot[b:e] if self._slot is not None else None,
        mask_bits=mask_bits, mu=mu, weight_decay=wd, grad_scale=scale, nesterov=self._nesterov)

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
    self._ensure_lr_buffers()
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
    self._ensure_lr_buffers()
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
    ops.masked_adam(g.W[b:e], g.G[b:e], self._slot[b:e], self._slot_v[b:e], self._beta_powers, lr,
                    lr_device=self._lr_dev if lr is None else None, beta1=self._beta1, beta2=self._beta2,
                    epsilon=self._epsilon, mask_bits=mask_bits, weight_decay=wd, grad_scale=scale)

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

  Not combined with data parallelism yet: an enabled GradSync (world > 1) raises NotImplementedError -- its bucket exchange
  starts inside every backward pass and would have to be held back to the last micro-batch; that is a follow-up."""

  def __init__(self, loss_fn, optimizer, micro_batches):
    k = int(micro_batches)
    if k < 1 or k != micro_batches:
      raise ValueError('micro_batches must be an integer >= 1, got %r' % (micro_batches,))
    inner = getattr(optimizer, '_optimizer', optimizer)
    if not hasattr(inner, '_accum'):
      raise TypeError('%s cannot accumulate (expected a rigl_amd.train optimizer or a wrapper around one)' % type(inner).__name__)
    sync = getattr(inner, '_grad_sync', None)
    if sync is not None and getattr(sync, 'enabled', False):
      raise NotImplementedError('MicroBatches with an enabled GradSync (world > 1): accumulation is not combined with the '
                                'in-backward bucket exchange yet')
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
    if not (torch.is_tensor(loss) and loss.is_cuda and loss.dtype == torch.float32 and loss.numel() == 1):
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
    inner._backward_done_for = None                     # pylint: disable=protected-access
    for i in range(self.micro_batches - 1):
      loss = self._loss_fn(*args, **kwargs)
      scalar = self._check_loss(loss)
      g.zero_other_grads()
      loss.backward()
      ops.grad_accumulate(self._arena, g.G, _lib.ACC_FIRST if i == 0 else _lib.ACC_ADD,
                          loss=scalar, loss_acc=self._loss_acc)
      del loss, scalar
    loss = self._loss_fn(*args, **kwargs)
    self._check_loss(loss)
    self._pending = loss
    inner._accum = self                                 # pylint: disable=protected-access
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

  def finished_for(self, loss):
    return loss is not None and self._done_for is loss

  def release(self):
    """The update was applied: the step's loss is let go of (see __call__)."""
    self._done_for = None

  def covers(self, loss):
    """True when ``loss`` has a pending or finished accumulation: its record's loss is ``self.loss``."""
    return loss is not None and (self._pending is loss or self._done_for is loss)


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
  ONE graph, keyed on the schedule object, is replayed through warm-up, drops and restarts alike.  A replay
  moves the optimizer's host mirror of that counter together with the global step; when the two disagree
  (``global_step.assign``, a checkpoint restore) the call runs eagerly, which uploads the counter -- a graph is
  never replayed against a stale counter.  The loss tensor returned is the captured step's output buffer.

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
    inner = getattr(optimizer, '_optimizer', optimizer)
    self._inner = inner
    sync = getattr(inner, '_grad_sync', None)
    self._eager_only = (sync is not None and getattr(sync, 'enabled', False)) or not torch.cuda.is_available()
    self.replays = 0
    self.eager_steps = 0
    self._ws_gen = ops.WORKSPACE_GENERATION
    self._last_key = None      # learning-rate key of the previous ordinary step and how many steps it has been stable
    self._stable = 0
    self._summ = getattr(inner, '_summary_hook', None)   # the summaries hook the cached graphs were captured with
    self._stable_needed = 1    # capture at the second consecutive ordinary step with the same learning rate

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
    inner = self._inner
    dev_lr = inner.lr_on_device() if hasattr(inner, 'lr_on_device') else False
    if dev_lr:
      if inner._lr_step is None or _int32(self._gs.value) != inner._lr_mirror:   # pylint: disable=protected-access
        return self._eager()                                       # allocates / uploads the device counter (never in a graph)
      key = inner._lr                                              # pylint: disable=protected-access
    else:
      key = _lr_value(inner._lr, self._gs)                         # pylint: disable=protected-access
    # attached training summaries keep a device step counter too, under the same protocol: a stale one is uploaded by an eager
    # call, and graphs captured with another hook (or none) enqueue another set of launches
    summ = getattr(inner, '_summary_hook', None)
    if summ is not self._summ:
      self._graphs.clear()
      self._summ = summ
    if summ is not None and _int32(self._gs.value) != summ.mirror:
      return self._eager()
    if self._ws_gen != ops.WORKSPACE_GENERATION:
      # a scratch buffer was (re)allocated since the graphs were captured (an eager mask update outgrew one, typically):
      # EVERY cached graph may point at the old buffer -- drop them all and capture again.  Checked before every replay,
      # so no graph is ever replayed against a freed buffer (ops.workspace keeps nothing alive for them).
      self._graphs.clear()
      self._ws_gen = ops.WORKSPACE_GENERATION
    ent = self._graphs.get(key)
    if ent is None:
      #  a learning rate that changes every step (linear warm-up, cosine) never reuses a graph keyed on its
      # value: while the key keeps changing, run plain eager steps and do not capture; once it has been stable for
      # `_stable_needed` consecutive steps (the constant plateaus of a piecewise schedule), capture again.
      if not dev_lr:                                               # (the device path has one key for the whole schedule)
        if key == self._last_key:
          self._stable += 1
        else:
          self._stable = 0
          self._last_key = key
        if self._stable < self._stable_needed:
          return self._eager()
      if self._warmup > 0:                                         # allocator / workspace caches / descriptors settle first
        self._warmup -= 1
        return self._eager()
      side = torch.cuda.Stream()
      side.wait_stream(torch.cuda.current_stream())
      with torch.cuda.stream(side):
        out = self._eager()                                        # THIS call's step, on a side stream as torch's capture recipe asks
      torch.cuda.current_stream().wait_stream(side)
      torch.cuda.synchronize()
      if self._is_update() or (not dev_lr and _lr_value(inner._lr, self._gs) != key):   # pylint: disable=protected-access
        return out                                                 # the next iteration is not an ordinary one at this lr: capture later
      gen0 = ops.WORKSPACE_GENERATION
      step1 = self._gs.value
      graph = torch.cuda.CUDAGraph()
      with torch.cuda.graph(graph):
        loss = self._loss_fn()
        self._opt.minimize(loss, self._gs)                         # capture enqueues nothing; undo its host side effect:
      self._gs.value = step1
      if dev_lr:
        inner._advance_lr_mirror(-1)                               # pylint: disable=protected-access
      if summ is not None:
        summ.advance_mirror(-1)
      if gen0 != ops.WORKSPACE_GENERATION or gen0 != self._ws_gen:
        # a buffer grew during the pre-capture step or the capture itself: graphs cached under other learning rates are
        # stale, and this one may hold both addresses -- keep none, the next call captures on settled buffers
        self._graphs.clear()
        self._ws_gen = ops.WORKSPACE_GENERATION
        return out
      if len(self._graphs) >= 16:
        self._graphs.pop(next(iter(self._graphs)))                 # bound the cache (piecewise-constant schedules have few values)
      self._graphs[key] = (graph, loss)
      return out
    graph, loss = ent
    if not dev_lr:
      self._last_key, self._stable = key, self._stable_needed
    graph.replay()
    self._gs.value += 1
    if dev_lr:
      inner._advance_lr_mirror(1)                                  # pylint: disable=protected-access
    if summ is not None:
      summ.advance_mirror(1)                                       # the replay wrote this step's record
    self._inner.graph.shadows_dirty = True                        # the replayed update rewrote the weights
    self.replays += 1
    return loss
