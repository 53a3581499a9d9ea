"""tf.contrib.model_pruning.python.pruning over the default graph: the getters
PruningGetterTf1Mixin calls (rigl/sparse_optimizers.py:46-56), and gradual
magnitude pruning (Zhu & Gupta), the 'prune' training_method of
rigl/mnist/mnist_train_eval.py:96-100, 320-337 and
rigl/cifar_resnet/resnet_train_eval.py:85, 249-275.

The reference only calls contrib; TF 1.15's contrib/model_pruning/python/pruning.py
is restated here, not executed (the status tests/golden/tf_shim.py has):

* schedule at step t, b = sparsity_function_begin_step, e = ..._end_step (fp32):
    p = min(1, max(0, f32(t - b) / f32(e - b)))
    s = f32(initial_sparsity - target_sparsity) * powf(1 - p, f32(exponent)) + target_sparsity
* a layer whose weight op name (``layer2/weights``) contains a weight_sparsity_map
  entry's name uses s_l = s * (f32(value) / f32(target_sparsity)); two matches
  raise ValueError; no match uses s.
* conditional_mask_update_op updates when t >= begin_pruning_step, t <=
  end_pruning_step (or end_pruning_step < 0) and last_mask_update_step +
  pruning_frequency <= t; an update sets last_mask_update_step = t.
* per masked layer (n weights, raw W): k = round_half_even(f32(n) * (1 - s_l))
  (k == 0 raises ValueError, as TF's gather(values, -1) fails), cur = the k-th
  largest |W|, thr = f32(cur * f32(1 - decay)) + f32(thr * f32(decay)),
  mask = |W| >= thr (ties all admitted).  Weights and slots are not touched.

The host evaluates the gate, the schedule and every k (it owns the global step);
the update itself is one rigl_magnitude_prune_batched call for all masked layers.
"""
import re

import numpy as np
import torch

from rigl_amd import ops
from rigl_amd import variables as V

_f32 = np.float32


def get_weights(graph=None):
  return (graph or V.get_default_graph()).get_weights()


def get_masks(graph=None):
  return (graph or V.get_default_graph()).get_masks()


def get_masked_weights(graph=None):
  """mask * W per layer (materialised on request; the kernels never need it)."""
  g = graph or V.get_default_graph()
  return [l.mask.data * l.weights.data for l in g.masked_layers()]


# ---- hyperparameters (tf.contrib.training.HParams subset) ------------------------------------------------------------
_PARAM_RE = re.compile(r'(?P<name>[a-zA-Z][\w\.]*)\s*=\s*((?P<val>[^,\[]*)|\[(?P<vals>[^\]]*)\])(,|$)')


class HParams:
  """Named hyperparameters typed by their defaults (tf.contrib.training.HParams): ``parse("a=1,b=[x,y]")``,
  ``set_hparam``, attribute access.  An unknown name raises ValueError."""

  def __init__(self, **defaults):
    self._values = dict(defaults)

  def __getattr__(self, name):
    values = self.__dict__.get('_values', {})
    if name in values:
      return values[name]
    raise AttributeError(name)

  @staticmethod
  def _cast(name, default, value):
    if isinstance(default, list):
      if not isinstance(value, (list, tuple)):
        raise ValueError('%s: expected a list, got %r' % (name, value))
      return [str(v) for v in value]
    if isinstance(default, bool):
      if isinstance(value, str):
        low = value.strip().lower()
        if low in ('true', '1'):
          return True
        if low in ('false', '0'):
          return False
        raise ValueError('%s: cannot parse %r as a bool' % (name, value))
      if isinstance(value, (bool, np.bool_)):
        return bool(value)
      raise ValueError('%s: expected a bool, got %r' % (name, value))
    if isinstance(default, int):
      if isinstance(value, str):
        return int(value.strip())
      if isinstance(value, bool) or not float(value).is_integer():
        raise ValueError('%s: expected an int, got %r' % (name, value))
      return int(value)
    if isinstance(default, float):
      return float(value.strip() if isinstance(value, str) else value)
    return str(value)

  def set_hparam(self, name, value):
    if name not in self._values:
      raise ValueError('Unknown hyperparameter %r' % name)
    self._values[name] = self._cast(name, self._values[name], value)

  def parse(self, values):
    """Overrides from a "name=value,name=[a,b]" string; returns self."""
    pos = 0
    values = values.strip()
    while pos < len(values):
      m = _PARAM_RE.match(values, pos)
      if not m:
        raise ValueError('Malformed hyperparameter value: %r' % values[pos:])
      pos = m.end()
      name = m.group('name')
      if name not in self._values:
        raise ValueError('Unknown hyperparameter %r' % name)
      if m.group('vals') is not None:
        vals = m.group('vals').strip()
        self.set_hparam(name, [v.strip() for v in vals.split(',')] if vals else [])
      else:
        if isinstance(self._values[name], list):
          raise ValueError('%s: expected a [list]' % name)
        self.set_hparam(name, m.group('val'))
    return self

  def values(self):
    return dict(self._values)

  def __repr__(self):
    return 'HParams(%s)' % ', '.join('%s=%r' % kv for kv in sorted(self._values.items()))


def get_pruning_hparams():
  """contrib's defaults.  ``prune_option`` (contrib's selector of the pruning score) is kept so that anything other
  than plain weight magnitude can be refused."""
  return HParams(
      name='model_pruning',
      begin_pruning_step=0,
      end_pruning_step=-1,
      weight_sparsity_map=[''],
      threshold_decay=0.0,
      pruning_frequency=10,
      nbins=256,
      block_height=1,
      block_width=1,
      block_pooling_function='AVG',
      initial_sparsity=0.0,
      target_sparsity=0.5,
      sparsity_function_begin_step=0,
      sparsity_function_end_step=100,
      sparsity_function_exponent=3,
      use_tpu=False,
      prune_option='weight')


# ---- host arithmetic (fp32, each operation rounded) -----------------------------------------------------------------
def schedule_sparsity(spec, step):
  """contrib Pruning._setup_sparsity at global step ``step`` (np.float32)."""
  b, e = int(spec.sparsity_function_begin_step), int(spec.sparsity_function_end_step)
  with np.errstate(divide='ignore', invalid='ignore'):
    p = np.minimum(_f32(1), np.maximum(_f32(0), _f32(step - b) / _f32(e - b)))
    return _f32(_f32(spec.initial_sparsity - spec.target_sparsity) *
                np.power(_f32(1) - p, _f32(spec.sparsity_function_exponent)) + _f32(spec.target_sparsity))


def parse_weight_sparsity_map(entries):
  """['name:value', ...] -> {name: float}; empty entries are skipped."""
  out = {}
  for entry in entries:
    if not entry:
      continue
    name, value = entry.split(':')
    out[name] = float(value)
  return out


def layer_sparsity(spec, sparsity_map, weight_name, s):
  """s_l of the weight op ``weight_name`` (substring match on the map's names)."""
  hits = [v for name, v in sparsity_map.items() if name in weight_name]
  if not hits:
    return _f32(s)
  if len(hits) > 1:
    raise ValueError('Multiple matches in weight_sparsity_map for weight %s' % weight_name)
  return _f32(_f32(s) * (_f32(hits[0]) / _f32(spec.target_sparsity)))


def num_kept(n, s_l):
  """k = round_half_even(f32(n) * (1 - s_l)); k == 0 fails as contrib's gather(values, -1) does."""
  k = int(np.rint(_f32(_f32(n) * (_f32(1) - _f32(s_l)))))
  if k < 1 or k > n:
    raise ValueError('pruning: k = %d for a tensor of %d weights at sparsity %r (contrib gathers values[k - 1])'
                     % (k, n, float(s_l)))
  return k


def weight_op_name(var):
  return var.name.split(':')[0]


# ---- state ----------------------------------------------------------------------------------------------------------
class PruningState:
  """What contrib adds to a graph: ``{scope}/threshold`` (fp32 scalar per masked layer, initially 0) and
  ``model_pruning/last_mask_update_step`` (int32).  Thresholds live in one device tensor, one slot per masked layer;
  the step is host state (the gate is host arithmetic)."""

  def __init__(self, graph, name):
    self.name = name
    self.scopes = [l.scope for l in graph.masked_layers()]
    self.thresholds = torch.zeros(len(self.scopes), dtype=torch.float32, device=graph.device)
    self.last_mask_update_step = torch.zeros((), dtype=torch.int32)

  def threshold_views(self):
    return [self.thresholds[i] for i in range(len(self.scopes))]

  def variable_items(self):
    """{contrib variable name: 0-d tensor} for checkpoints."""
    out = {'%s/threshold' % scope: self.thresholds[i] for i, scope in enumerate(self.scopes)}
    out['%s/last_mask_update_step' % self.name] = self.last_mask_update_step
    return out


def _pruning_state(graph, name='model_pruning', create=False):
  st = getattr(graph, 'pruning_state', None)
  if st is None and create:
    graph.finalize()
    st = graph.pruning_state = PruningState(graph, name)
  return st


def get_thresholds(graph=None):
  """The per-layer thresholds (0-d device views), in get_masks() order; [] before a Pruning object exists."""
  st = _pruning_state(graph or V.get_default_graph())
  return st.threshold_views() if st is not None else []


def get_weight_sparsity(graph=None):
  """Fraction of zeros of every mask (nn_impl.zero_fraction), np.float32 each."""
  return [_f32(1) - _f32(_f32(m.sum()) / _f32(m.numel)) for m in get_masks(graph)]


class Pruning:
  """contrib Pruning(spec, global_step, sparsity): gradual magnitude pruning of every masked layer of ``graph``.

  The drivers run ``conditional_mask_update_op`` under control_dependencies([train_op]), so here it is called after
  the training step, and the step it sees (for the gate AND the schedule) is the global step the training step has
  already incremented.  (TF1 does not order the schedule's read of the step against that increment; reading the
  incremented step is the choice pinned here.)  ``sparsity``: a fixed fp32 sparsity in place of the schedule.
  """

  def __init__(self, spec=None, global_step=None, sparsity=None, graph=None):
    self._graph = graph or V.get_default_graph()
    self._spec = spec if spec is not None else get_pruning_hparams()
    sp = self._spec
    if int(sp.block_height) != 1 or int(sp.block_width) != 1:
      raise NotImplementedError('block pruning (block_height=%d, block_width=%d)' % (sp.block_height, sp.block_width))
    if sp.use_tpu:
      raise NotImplementedError('use_tpu=True (the histogram threshold path)')
    if sp.prune_option != 'weight':
      raise NotImplementedError('prune_option=%r: only weight magnitude is restated' % sp.prune_option)
    self._global_step = global_step if global_step is not None else self._graph.get_or_create_global_step()
    self._fixed_sparsity = None if sparsity is None else _f32(sparsity)
    self._map = parse_weight_sparsity_map(sp.weight_sparsity_map)
    self._state = _pruning_state(self._graph, sp.name, create=True)
    self._counts = None

  @property
  def sparsity(self):
    """The schedule's sparsity at the current global step (np.float32)."""
    if self._fixed_sparsity is not None:
      return self._fixed_sparsity
    return schedule_sparsity(self._spec, int(self._global_step))

  def layer_ks(self, step=None):
    """[(masked layer, k)] at ``step`` (default: the current global step)."""
    s = self.sparsity if step is None else (
        self._fixed_sparsity if self._fixed_sparsity is not None else schedule_sparsity(self._spec, step))
    out = []
    for l in self._graph.masked_layers():
      s_l = layer_sparsity(self._spec, self._map, weight_op_name(l.weights), s)
      out.append((l, num_kept(l.weights.numel, s_l)))
    return out

  def should_update(self, step=None):
    sp = self._spec
    t = int(self._global_step) if step is None else int(step)
    in_range = t >= sp.begin_pruning_step and (t <= sp.end_pruning_step or sp.end_pruning_step < 0)
    return bool(in_range and int(self._state.last_mask_update_step) + sp.pruning_frequency <= t)

  def mask_update_op(self, counts=False):
    """Updates every mask and threshold now; last_mask_update_step = the global step.  ``counts=True`` returns the
    device int32 [n_layers, 4] (n, k, new ones, old ones)."""
    g = self._graph
    g.finalize()
    t = int(self._global_step)
    items = [(l.weights.data.view(-1), l.mask.bits, self._state.thresholds[i:i + 1], k)
             for i, (l, k) in enumerate(self.layer_ks(t))]
    out = None
    if counts:
      out = torch.empty((len(items), 4), dtype=torch.int32, device=g.device)
    ops.magnitude_prune_batched(items, self._spec.threshold_decay, out)
    self._state.last_mask_update_step.fill_(t)
    g.shadows_dirty = True              # the next forward re-packs bf16(mask * W), eager or replayed
    return out

  def conditional_mask_update_op(self):
    """Runs mask_update_op when the gate holds; returns whether it ran (the masks were rewritten)."""
    if not self.should_update():
      return False
    self.mask_update_op()
    return True
