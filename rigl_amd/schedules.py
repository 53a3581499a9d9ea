"""The reference's learning-rate schedules, with two faces.

  host    ``sched(step) -> float``: the fp32 operations of the TF graph, one rounding each, in NumPy.  Usable wherever a
          callable learning rate is accepted.
  device  ``sched.descriptor()``: the RiglLrSchedule table ``ops.lr_schedule_step`` evaluates on the GPU
          (rigl_lr_schedule_step, include/rigl_hip.h).  An optimizer of rigl_amd.train given a ``Schedule`` keeps the step
          counter and the rate in device memory, so ``train.GraphedStep`` replays ONE graph through the whole schedule
          instead of running eager steps while the rate changes.

``sched.host_only()`` is the same function as a plain callable: the optimizers then take the host path (A/B runs).

The table: at most 32 segments in ascending ``start`` order; the active one is the LAST with ``!(x < start)`` (below every
start: the first), where x is the int32 step (step domain, integer comparison) or f32(step) / f32(steps_per_epoch) (epoch
domain, imagenet_train_eval.py:352-353).  That is what the reference's chain ``rate = tf.where(x < start, rate, const)``
(:327-329) ends with for ascending starts.  Kinds (every operation rounded to fp32 separately):
  CONST   lr = c
  WARMUP  lr = (c * x) / d                                                                  (:325-326)
  COSINE  frac = ((x / d) - sum_r) / len;  lr = c * ((0.5 * m_fac) * (1 + f32(cos(double(f32(pi) * frac)))))
          -- one cycle of TF 1.15's cosine_decay_restarts (alpha = 0); sum_r, len and m_fac are the cycle's constants.
"""
import math

import numpy as np

from rigl_amd import _lib

_F = np.float32
_PI32 = _F(math.pi)
_INT32_MIN, _INT32_MAX = -2 ** 31, 2 ** 31 - 1
MAX_SEGMENTS = _lib.LR_MAX_SEGMENTS
STEP, EPOCH = _lib.LR_DOMAIN_STEP, _lib.LR_DOMAIN_EPOCH
CONST, WARMUP, COSINE = _lib.LR_CONST, _lib.LR_WARMUP, _lib.LR_COSINE


def _seg(kind, start, c, d=0.0, sum_r=0.0, length=1.0, m_fac=1.0):
  return dict(kind=kind, start=start, c=_F(c), d=_F(d), sum_r=_F(sum_r), len=_F(length), m_fac=_F(m_fac))


def _cosine_value(c, d, sum_r, length, m_fac, x):
  """One COSINE segment at x (fp32 scalars in, fp32 out): the operation order of the kernel."""
  frac = (x / d - sum_r) / length
  t = _PI32 * frac
  cs = _F(np.cos(np.float64(t)))
  return c * ((_F(0.5) * m_fac) * (_F(1.0) + cs))


class Schedule:
  """A segment table (see the module docstring).  ``segments``: dicts from ``_seg``; ``start`` is an int (step domain) or a
  float (epoch domain); the first segment's start is ignored (it is active below every other start)."""

  def __init__(self, domain, segments, steps_per_epoch=None, name='lr_schedule'):
    segments = list(segments)
    if not 1 <= len(segments) <= MAX_SEGMENTS:
      raise ValueError('%s: %d segments, the device table holds 1..%d' % (name, len(segments), MAX_SEGMENTS))
    if domain not in (STEP, EPOCH):
      raise ValueError('%s: unknown domain %r' % (name, domain))
    self.domain = domain
    self.name = name
    self.steps_per_epoch = None
    if domain == EPOCH:
      spe = _F(steps_per_epoch)
      if not (np.isfinite(spe) and spe > 0):
        raise ValueError('%s: steps_per_epoch must be finite and > 0, got %r' % (name, steps_per_epoch))
      self.steps_per_epoch = spe
    segs = []
    for i, s in enumerate(segments):
      s = dict(s)
      if domain == STEP:
        st = _INT32_MIN if i == 0 else int(s['start'])
        if st != s['start'] and i > 0:
          raise ValueError('%s: segment %d: a step-domain start must be an integer, got %r' % (name, i, s['start']))
        if not _INT32_MIN <= st <= _INT32_MAX:
          raise ValueError('%s: segment %d: start %d does not fit int32' % (name, i, st))
      else:
        st = _F(-np.inf) if i == 0 else _F(s['start'])
        if np.isnan(st):
          raise ValueError('%s: segment %d: NaN start' % (name, i))
      if i > 0 and st < segs[-1]['start']:
        raise ValueError('%s: segment starts must ascend (%r after %r)' % (name, st, segs[-1]['start']))
      if s['kind'] not in (CONST, WARMUP, COSINE):
        raise ValueError('%s: segment %d: unknown kind %r' % (name, i, s['kind']))
      if s['kind'] == COSINE and not s['len'] > 0:
        raise ValueError('%s: segment %d: a COSINE cycle length must be > 0' % (name, i))
      s['start'] = st
      segs.append(s)
    self.segments = segs
    self._desc = None

  # ---- host ----------------------------------------------------------------------------------------------------------
  def active_segment(self, step):
    """(index of the active segment, x) at ``step`` (an int32 counter: wraps as the device's does)."""
    s = (int(step) - _INT32_MIN) % 2 ** 32 + _INT32_MIN
    x = _F(s)
    if self.domain == EPOCH:
      x = x / self.steps_per_epoch
    a = 0
    for i in range(1, len(self.segments)):
      below = (x < self.segments[i]['start']) if self.domain == EPOCH else (s < self.segments[i]['start'])
      if not below:
        a = i
    return a, x

  def value32(self, step):
    """np.float32 learning rate at ``step``: the bits the device writes."""
    a, x = self.active_segment(step)
    g = self.segments[a]
    if g['kind'] == WARMUP:
      return (g['c'] * x) / g['d']
    if g['kind'] == COSINE:
      return _cosine_value(g['c'], g['d'], g['sum_r'], g['len'], g['m_fac'], x)
    return g['c']

  def __call__(self, step):
    return float(self.value32(step))

  def host_only(self):
    """The same function as a plain callable: an optimizer given this evaluates it on the host every step and passes the
    rate by value (the path every callable takes)."""
    return lambda step: self(step)

  # ---- device --------------------------------------------------------------------------------------------------------
  def descriptor(self):
    """The RiglLrSchedule (an _lib.LrSchedule) of this schedule; built once."""
    if self._desc is None:
      d = _lib.LrSchedule()
      d.n_seg = len(self.segments)
      d.domain = self.domain
      d.steps_per_epoch = float(self.steps_per_epoch) if self.domain == EPOCH else 0.0
      for i, s in enumerate(self.segments):
        g = d.seg[i]
        g.kind = s['kind']
        if self.domain == STEP:
          g.start_step, g.start = s['start'], 0.0
        else:
          g.start_step, g.start = 0, float(s['start'])
        g.c, g.d, g.sum_r, g.len, g.m_fac = (float(s[k]) for k in ('c', 'd', 'sum_r', 'len', 'm_fac'))
      self._desc = d
    return self._desc


# ----------------------------------------------------------------------------------------------------------------------
# builders
# ----------------------------------------------------------------------------------------------------------------------
def piecewise_constant(boundaries, values, name='piecewise_constant'):
  """tf.train.piecewise_constant(global_step, boundaries, values) on the int32 step: values[0] while step <= boundaries[0],
  values[i] while boundaries[i-1] < step <= boundaries[i], values[-1] above the last boundary
  (resnet_train_eval.py:196-200, mnist_train_eval.py:253-256).  ``x <= b`` keeps the old value, so the segment of values[i]
  starts at the integer boundaries[i-1] + 1."""
  boundaries, values = list(boundaries), list(values)
  if len(values) != len(boundaries) + 1:
    raise ValueError('%s: %d values for %d boundaries (one more is needed)' % (name, len(values), len(boundaries)))
  for b in boundaries:
    if int(b) != b:
      raise ValueError('%s: boundaries are integer steps, got %r' % (name, b))
  if any(b1 < b0 for b0, b1 in zip(boundaries, boundaries[1:])):
    raise ValueError('%s: boundaries must be sorted, got %r' % (name, boundaries))
  segs = [_seg(CONST, 0, values[0])]
  segs += [_seg(CONST, int(b) + 1, v) for b, v in zip(boundaries, values[1:])]
  return Schedule(STEP, segs, name=name)


def cosine_decay(lr, decay_steps, name='cosine_decay'):
  """tf.train.cosine_decay(lr, global_step, decay_steps), alpha = 0: the one-cycle case of cosine_decay_restarts, held at its
  end value (global_step = min(global_step, decay_steps)) from ``decay_steps`` on."""
  if int(decay_steps) != decay_steps or decay_steps <= 0:
    raise ValueError('%s: decay_steps must be a positive integer, got %r' % (name, decay_steps))
  end = _cosine_value(_F(lr), _F(decay_steps), _F(0), _F(1), _F(1), _F(decay_steps))
  return Schedule(STEP, [_seg(COSINE, 0, lr, d=decay_steps), _seg(CONST, int(decay_steps), end)], name=name)


def cosine_decay_restarts(lr, first_decay_steps, t_mul=2.0, m_mul=1.0, total_steps=None, steps_per_epoch=None,
                          name='cosine_decay_restarts'):
  """tf.train.cosine_decay_restarts(lr, x, first_decay_steps, t_mul, m_mul), alpha = 0 (imagenet_train_eval.py:321-323), one
  COSINE segment per cycle.  TF 1.15, all fp32:
      completed = x / first_decay_steps
      i         = floor(log(1 - completed * (1 - t_mul)) / log(t_mul))       (t_mul == 1: floor(completed))
      sum_r     = (1 - t_mul ** i) / (1 - t_mul)                             (t_mul == 1: i)
      frac      = (completed - sum_r) / t_mul ** i                           (t_mul == 1: completed - i)
      lr        = lr * (0.5 * m_mul ** i * (1 + cos(pi * frac)))
  sum_r, t_mul ** i and m_mul ** i are written into the table here, in that order of operations; the cycle is chosen by the
  segment comparison against first_decay_steps * sum_r, so the device evaluates no log, pow or floor.  Cycles are emitted
  until ``total_steps`` (required) is covered; more than 32 raise.  ``steps_per_epoch``: x is the fp32 epoch (and
  ``first_decay_steps`` is in epochs) instead of the step."""
  if total_steps is None:
    raise ValueError('%s: total_steps is required (the table holds one segment per cycle of the run)' % name)
  if not first_decay_steps > 0 or not t_mul >= 1.0:
    raise ValueError('%s: first_decay_steps must be > 0 and t_mul >= 1' % name)
  epoch = steps_per_epoch is not None
  t, m, fds, one = _F(t_mul), _F(m_mul), _F(first_decay_steps), _F(1.0)
  segs = []
  i = 0
  while True:
    fi = _F(i)
    if t == one:
      sum_r, length = fi, one
    else:
      length = np.power(t, fi)
      sum_r = (one - length) / (one - t)
    start = fds * sum_r                                           # in x units (fp32), where completed == sum_r
    start_steps = float(start) * (float(_F(steps_per_epoch)) if epoch else 1.0)
    if i > 0 and start_steps >= total_steps:
      break
    if len(segs) == MAX_SEGMENTS:
      raise ValueError('%s: more than %d cycles before step %d' % (name, MAX_SEGMENTS, total_steps))
    segs.append(_seg(COSINE, float(start) if epoch else int(math.ceil(float(start))), lr, d=fds, sum_r=sum_r,
                     length=length, m_fac=np.power(m, fi)))
    i += 1
  return Schedule(EPOCH if epoch else STEP, segs, steps_per_epoch=steps_per_epoch, name=name)


def imagenet_lr_schedule(base_learning_rate, train_batch_size, num_train_images=1281167, model_architecture='resnet',
                         training_steps_multiplier=1.0, use_sgdr=False, sgdr_decay_step=5, sgdr_t_mul=1.5, sgdr_m_mul=.5,
                         train_steps=None):
  """set_lr_schedule + lr_schedule of imagenet_train_eval.py:280-330, on current_epoch = f32(step) / f32(num_train_images /
  train_batch_size) (:352-353):  a linear warm-up  scaled_lr * mult0 * epoch / start_epoch0  below the first start epoch,
  then  scaled_lr * mult  from each (mult, start_epoch) on; scaled_lr = base_learning_rate * (train_batch_size / 256).
  ``use_sgdr``: cosine_decay_restarts(scaled_lr, epoch, sgdr_decay_step, sgdr_t_mul, sgdr_m_mul) instead, which needs
  ``train_steps`` (the run's length BEFORE the multiplier, as the flag: :293 scales it)."""
  if model_architecture in ('mobilenet_v2', 'mobilenet_v1'):
    table = [(1.0, 8), (0.1, 40), (0.01, 75), (0.001, 95), (.0003, 120)]                       # :284
  elif model_architecture == 'resnet' or model_architecture.startswith('vgg'):
    table = [(1.0, 0), (0.1, 30), (0.01, 70), (0.001, 90), (.0001, 120)]                       # :287
  else:
    raise ValueError('Unknown architecture ' + model_architecture)
  if training_steps_multiplier != 1.0:
    table = [(x, y * training_steps_multiplier) for x, y in table]                             # :292
    if train_steps is not None:
      train_steps = int(train_steps * training_steps_multiplier)                               # :293
  steps_per_epoch = num_train_images / train_batch_size                                        # :352
  scaled_lr = base_learning_rate * (train_batch_size / 256.0)                                  # :319
  if use_sgdr:
    if train_steps is None:
      raise ValueError('imagenet_lr_schedule: use_sgdr needs train_steps (total_steps of cosine_decay_restarts)')
    return cosine_decay_restarts(scaled_lr, sgdr_decay_step, t_mul=sgdr_t_mul, m_mul=sgdr_m_mul, total_steps=train_steps,
                                 steps_per_epoch=steps_per_epoch, name='imagenet_sgdr')
  segs = [_seg(WARMUP, 0.0, scaled_lr * table[0][0], d=table[0][1])]                           # :325-326
  segs += [_seg(CONST, start_epoch, scaled_lr * mult) for mult, start_epoch in table]          # :327-329
  return Schedule(EPOCH, segs, steps_per_epoch=steps_per_epoch, name='imagenet_' + model_architecture)


def cifar_lr_schedule(training_steps_multiplier=1.0):
  """resnet_train_eval.py:189-200: 0.1 / 5**i, dropping after steps 30000, 60000 and 90000 (times the multiplier)."""
  boundaries = [30000, 60000, 90000]
  if training_steps_multiplier != 1.0:
    boundaries = [int(x * training_steps_multiplier) for x in boundaries]
  return piecewise_constant(boundaries, [0.1 / (5. ** i) for i in range(len(boundaries) + 1)], name='cifar_lr_schedule')


def mnist_lr_schedule(learning_rate, batch_per_epoch, use_model_pruning=False, lr_drop_epoch=75):
  """mnist_train_eval.py:249-256 (--optimizer != adam): learning_rate / 3**i, dropping after epochs 60, 70 and 80, or after
  lr_drop_epoch and lr_drop_epoch + 20 with model pruning."""
  if not use_model_pruning:
    boundaries = [int(round(s * batch_per_epoch)) for s in [60, 70, 80]]
  else:
    boundaries = [int(round(s * batch_per_epoch)) for s in [lr_drop_epoch, lr_drop_epoch + 20]]
  return piecewise_constant(boundaries, [learning_rate / (3. ** i) for i in range(len(boundaries) + 1)],
                            name='mnist_lr_schedule')
