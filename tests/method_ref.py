"""NumPy fp32 restatement of ONE optimizer call of every training method of rigl_amd/sparse_optimizers.py -- the yardstick
of tests/test_method_ref_cpu.py (which checks this file on its own) and tests/test_methods_gpu.py (which holds the device
to it bit for bit).  TEST INFRASTRUCTURE ONLY.

``step(cfg, arena, state, G, rand)`` is a pure function of the state before the call (weights, masks, slots, EMA shadows,
global step, last update step), the dense gradient arena of the call and the random tensors of the call.  It returns the
state after the call and what the call did.  Nothing is modified in place.

What is pinned elsewhere is used, not restated: oracle.rigl_oracle.get_update / masked_grad / momentum_apply / sgd_apply /
get_drop_fraction / is_mask_update_iter / get_n_zeros / topk_order / get_sparsities, tests/adam_ref.py and
oracle/tf_random.py.  New here is the ORDER of operations of a call, each stated with the reference lines it restates
(rigl/sparse_optimizers_base.py = "base", rigl/sparse_optimizers.py = "so"):

  SET family (base:118-187)   _before_apply_gradients (base:133) -> the inner optimizer's apply over EVERY variable, which
                              increments the step on every call (base:135-136) -> gate and update on the UPDATED weights and
                              slots with the INCREMENTED step (base:145-146, :184-186).  Seeds are
                              int32([offset + hash(name + tag), global_step]) (base:402-418).  Every slot of a new connection
                              is reset to zero (base:345-353).
  Static (so:109-123)         score_grow = mask, reinit_when_same=True.
  SNFS (so:176-214)           ema -= (1 - decay) * (ema - g), zero shadows, g the gradient w.r.t. mask*W -- the raw arena
                              gradient (so:189-192) --, updated before the apply (so:195-197); grow score |ema| (so:213).
  RigL (base:487-564)         a call is EITHER the apply or the update (base:508-521); an update call does not increment
                              the step.  Slots of new connections become grad * initial_acc_scale (base:555-564); grow
                              tensors base:355-400 + :540-553.
  SNIP (so:258-338)           at step 0, once: no apply, no increment; mask = top n_keep of |g * v| (so:301-316) with g the
                              gradient of the loss INCLUDING the regulariser w.r.t. the variable = mask*G + wd*W;
                              n_keep = n - get_n_zeros(n, s) (so:302-304) from get_sparsities.  Afterwards the inner optimizer.
  DNW (so:375-471)            gradients are taken w.r.t. the masked_weights tensors (so:379-386): G unmasked and no l2 on
                              the masked kernels; dense kernels keep their l2, BN / bias have none.  Then every mask is the
                              top n_keep of |W| (so:444-459), on every call.

Arena form.  The device keeps every variable in one flat fp32 arena (rigl_amd/variables.py); the state here has the same
form, so an arena segment is compared whole, padding included: ``W``, every slot and ``G`` are fp32 [total]; ``mask`` is
fp32 0/1 over the masked segment (0 in padding).  The inner optimizers are elementwise, so their restatement is one call over
the arena with a per-element mask (1 outside the masked segment) and a per-element weight decay.

Random tensors.  ``rand`` maps (seed0, seed1, dist) to dict(out=fp32 [n], scale=, shift=): what the device drew.  Uniform
tensors are always computed here from oracle.tf_random (the device is bit-exact there and the GPU test compares them);
``random_uniform_d``'s bounds (mean |W|, a reduction whose order is the device's) are read from the record.  Normal tensors
are taken from the record: ocml's sinf / cosf / logf are not glibc's and the ranking depends on every bit; the GPU test
holds them to the oracle's stream separately.  Without a record (the CPU tests) both come from oracle.tf_random.

The two reductions behind ``random_uniform_d`` / ``random_normal_d`` -- mean |W| and the population std of W, base:382 and
:390 -- are the one quantity NOT held bit for bit: the float64 value of each is logged with the draw (``expect``) and the GPU
test holds the device's value to it at ``reduction_bound(n)``, a bound derived from the fp32 format alone.

``mutant``: one of MUTANTS -- a deliberately wrong order of operations.  'ema_updated_after_the_update' is the issue's
"EMA updated after the apply": the EMA is a function of the gradients alone, so moving its update behind the apply changes
no value; what such an order gets wrong is that the update of the same call scores with the EMA of the call before, and
that is what the mutant does.  tests/test_method_ref_cpu.py requires the case set
to tell each one from the reference; this is a statement about the cases, not about the product.
"""
import os

import numpy as np

import adam_ref as A
from oracle import rigl_oracle as O
from oracle import tf_random as T

F32 = np.float32

SET_FAMILY = ('set', 'static', 'snfs')
METHODS = SET_FAMILY + ('rigl', 'snip', 'dnw')

MUTANTS = (
    'set_update_on_pre_apply_weights', 'seed_step_before_increment', 'grow_drop_tags_swapped', 'signed_ema_grow_score',
    'ema_updated_after_the_update', 'ema_of_masked_gradient', 'static_without_reinit', 'rigl_momentum_reset_in_set',
    'second_adam_slot_not_reset', 'dnw_l2_on_masked_kernels', 'dnw_masked_gradient', 'dnw_no_l2_on_dense_kernels',
    'dnw_scores_shifted_by_one', 'snip_score_without_wd', 'snip_increments_step', 'rigl_applies_on_update_call',
    'drop_noise_left_out')


def name_hash(text):
  """``hash(text)`` of the reference's process (base:270): the builtin under an integer PYTHONHASHSEED, else the value a
  PYTHONHASHSEED=0 CPython computes (oracle.tf_random.python_str_hash, pinned against the interpreter)."""
  if os.environ.get('PYTHONHASHSEED', '').isdigit():
    return hash(text)
  return T.python_str_hash(text, 0)


class Layer:
  """One masked kernel: ``name`` of the weights variable ('<scope>/weights:0'), its mask's, arena offset, size."""

  def __init__(self, scope, offset, shape):
    self.scope = scope
    self.name = scope + '/weights:0'
    self.mask_name = scope + '/mask:0'
    self.offset = int(offset)
    self.shape = tuple(int(s) for s in shape)
    self.numel = int(np.prod(self.shape))

  @property
  def sl(self):
    return slice(self.offset, self.offset + self.numel)


class Arena:
  """Layout: ``total`` elements, the masked segment is [0, n_masked), the dense-kernel segment [n_masked, n_kernel), BN and
  biases behind it; ``wd`` fp32 [total] per-element weight decay (0 in padding and on BN / biases); ``layers`` in creation
  order."""

  def __init__(self, total, n_masked, n_kernel, wd, layers):
    self.total, self.n_masked, self.n_kernel = int(total), int(n_masked), int(n_kernel)
    self.wd = np.asarray(wd, F32)
    self.layers = list(layers)
    assert self.wd.shape == (self.total,)

  def mask_shapes(self):
    from collections import OrderedDict
    return OrderedDict((l.mask_name, l.shape) for l in self.layers)


class Cfg:
  """The constructor arguments of the optimizer under test and of its inner optimizer."""

  def __init__(self, method, inner='sgd', lr=0.1, mu=0.9, nesterov=True, beta1=0.9, beta2=0.999, epsilon=1e-8, begin=0, end=-1,
               frequency=1, drop_fraction=0.1, anneal='constant', grow_init='zeros', initial_acc_scale=0., noise_std=1e-5,
               seed_offset=0, ema_decay=0.9, default_sparsity=0.5, mask_init_method='random', custom_sparsity_map=None):
    assert method in METHODS and inner in ('sgd', 'momentum', 'adam')
    self.method, self.inner = method, inner
    self.lr, self.mu, self.nesterov = lr, mu, nesterov
    self.beta1, self.beta2, self.epsilon = beta1, beta2, epsilon
    self.begin, self.end, self.frequency = int(begin), int(end), int(frequency)
    self.drop_fraction, self.anneal = drop_fraction, anneal
    self.grow_init, self.initial_acc_scale = grow_init, initial_acc_scale
    self.noise_std, self.seed_offset, self.ema_decay = noise_std, int(seed_offset), ema_decay
    self.default_sparsity, self.mask_init_method = default_sparsity, mask_init_method
    self.custom_sparsity_map = dict(custom_sparsity_map or {})

  def n_slots(self):
    return {'sgd': 0, 'momentum': 1, 'adam': 2}[self.inner]


def initial_state(cfg, arena, W, mask):
  """The state in front of the first call: zero slots (created at zero by the inner optimizers), beta powers (beta1, beta2)
  (tf.train.AdamOptimizer._create_slots), no EMA shadow yet (zero, so:173), step 0, last update -frequency (base:164-171)."""
  return dict(W=np.array(W, F32), mask=np.array(mask, F32),
              slots=tuple(np.zeros(arena.total, F32) for _ in range(cfg.n_slots())),
              beta_powers=np.array([cfg.beta1, cfg.beta2], F32) if cfg.inner == 'adam' else None,
              ema={}, gs=0, last_update_step=-cfg.frequency, is_snipped=False)


# ------------------------------------------------------------------------------------------------ the inner optimizer
def inner_apply(cfg, arena, st, G, mask_full, wd):
  """One apply_gradients of the inner optimizer over the whole arena: g = mask * G + wd * W (oracle.masked_grad), then
  tf.train.GradientDescentOptimizer / MomentumOptimizer (oracle.sgd_apply / momentum_apply) / AdamOptimizer (adam_ref, both
  slots, the beta powers advanced once behind every variable's update).  Returns (W, slots, beta_powers)."""
  W = st['W']
  if cfg.inner == 'adam':
    g = A.masked_grad(G, mask_full, W, wd)
    w, m, v = A.adam_apply(W, st['slots'][0], st['slots'][1], g, cfg.lr, st['beta_powers'], cfg.beta1, cfg.beta2, cfg.epsilon)
    return w, (m, v), A.advance(st['beta_powers'], cfg.beta1, cfg.beta2)
  g = O.masked_grad(G, mask_full, W, wd)
  if cfg.inner == 'momentum':
    w, a = O.momentum_apply(W, st['slots'][0], g, cfg.lr, cfg.mu, nesterov=cfg.nesterov)
    return w, (a,), None
  return O.sgd_apply(W, g, cfg.lr), (), None


def _full_mask(arena, mask):
  m = np.ones(arena.total, F32)
  m[:arena.n_masked] = mask
  return m


# ------------------------------------------------------------------------------------------------ random tensors
class _Draws:

  def __init__(self, cfg, rand, strict):
    self.cfg, self.rand, self.strict = cfg, rand or {}, strict
    self.recorded = bool(strict or rand)      # the device's records are the source of reduction-derived bounds
    self.log = []

  def __call__(self, layer, tag, dist, step, scale=None, shift=None, expect=None):
    """stateless_random_{uniform|normal}(shape, seed=int32([offset + hash(name + tag), step])) * scale + shift
    (base:402-418).  ``scale`` None: read from the device's record (a reduction of the device's); ``expect`` is then the
    float64 value of that reduction, logged for the caller to hold the record to (reduction_bound)."""
    s0, s1 = T.tf_seed_pair(self.cfg.seed_offset, name_hash(layer.name + tag), step)
    rec = self.rand.get((s0, s1, dist))
    if rec is None and self.strict:
      raise AssertionError('%s: no %s tensor with seed (%d, %d) = (offset + hash(name + %r), step %d) was drawn'
                           % (layer.scope, dist, s0, s1, tag, step))
    if scale is None:
      scale, shift = rec['scale'], rec['shift']
    n = layer.numel
    if dist == 'uniform':
      rnd = T.stateless_random_uniform(n, s0, s1)                          # [0, 1)
      out = ((rnd * F32(scale)).astype(F32) + F32(shift)).astype(F32)      # rnd * (maxval - minval) + minval
    elif rec is not None:
      out = np.asarray(rec['out'], F32).reshape(-1)
    else:
      out = T.stateless_random_normal(n, s0, s1, 0.0, scale)
    assert out.shape == (n,)
    self.log.append(dict(layer=layer.scope, tag=tag, dist=dist, seed=(s0, s1), step=step, n=n, scale=float(scale),
                         shift=float(shift or 0.0), value=out, expect=expect))
    return out


# ------------------------------------------------------------------------------------------------ the mask update
def _ties_admitted(score, idx, k):
  """The update's counts 5 / 6: how many of the k selected entries carry the threshold's score."""
  n = score.size
  if k <= 0 or n == 0:
    return 0
  if k >= n:
    return n
  return int((score[idx[:k]] == score[idx[k - 1]]).sum())


def _grow_tensor(cfg, layer, w, g, draw, step):
  """base:355-400 and, for RigL, :540-553.  None = zeros."""
  method = cfg.grow_init
  if method == 'zeros':
    return None
  if cfg.method == 'rigl' and method.startswith(('grad_scale', 'grad_sign')):
    return O.get_grow_tensor_rigl(w, g, method)
  div = F32(O.extract_number(method))
  if method.startswith('random_uniform'):                       # base:389-397: minval = -mean |W|, maxval = mean |W|
    mean64 = float(np.mean(np.abs(w.astype(np.float64))))
    if draw.recorded:
      t = draw(layer, 'grow_init_u', 'uniform', step, expect=mean64)
    else:
      mean = F32(mean64)
      t = draw(layer, 'grow_init_u', 'uniform', step, F32(mean) - F32(-mean), -mean)
    return (t / div).astype(F32)
  if method.startswith('random_normal'):                        # base:381-388: stddev = reduce_std(W), the population's
    std64 = float(np.std(w.astype(np.float64)))
    std = None if draw.recorded else F32(std64)
    return (draw(layer, 'grow_init_n', 'normal', step, std, 0.0 if std is not None else None, expect=std64) / div).astype(F32)
  raise ValueError('Grow-Init: %s is not a valid option.' % method)


def mask_update(cfg, arena, W, mask, slots, G, ema, frac, step, draw, mutant=None, W_scores=None, ema_scores=None):
  """cond_mask_update_op's true branch (base:173-182): generic_mask_update + _get_update_op + reset_momentum of every layer,
  at seed step ``step``.  Returns (W, mask, slots, counts [n_layers, 8], per-layer facts)."""
  W, mask = W.copy(), mask.copy()
  slots = tuple(s.copy() for s in slots)
  rigl = cfg.method == 'rigl'
  counts, facts = [], []
  tag_drop, tag_grow = ('grow', 'drop') if mutant == 'grow_drop_tags_swapped' else ('drop', 'grow')
  for l in arena.layers:
    w, m, g = W[l.sl].copy(), mask[l.sl].copy(), G[l.sl]
    noise = None
    if cfg.noise_std and mutant != 'drop_noise_left_out':
      noise = draw(l, tag_drop, 'normal', step, cfg.noise_std, 0.0)
    # score_drop = |mask * W| + noise (base:263-270, so:112-119, so:202-210, base:526-534)
    sd = O.rigl_scores(m, w if W_scores is None else W_scores[l.sl], g, noise)[0]
    reinit = False
    if cfg.method == 'set':
      sg = draw(l, tag_grow, 'uniform', step, 1.0, 0.0)                     # base:272-273
    elif cfg.method == 'static':
      sg, reinit = m.copy(), mutant != 'static_without_reinit'              # so:121-123
    elif cfg.method == 'snfs':
      e = (ema if ema_scores is None else ema_scores).get(l.name)
      e = np.zeros(l.numel, F32) if e is None else e
      sg = e if mutant == 'signed_ema_grow_score' else np.abs(e)            # so:213
    else:
      sg = np.abs(g)                                                         # base:535-536
    r = O.get_update(sd, sg, m, w, frac, grow_tensor=_grow_tensor(cfg, l, w, g, draw, step), reinit_when_same=reinit)
    new_conn = r['new_connections'].reshape(-1)
    if rigl or mutant == 'rigl_momentum_reset_in_set':                       # base:555-564
      acc = (g * F32(cfg.initial_acc_scale)).astype(F32)
    else:                                                                    # base:345-353
      acc = np.zeros(l.numel, F32)
    for i, s in enumerate(slots):
      if i == 1 and mutant == 'second_adam_slot_not_reset':
        continue
      s[l.sl] = np.where(new_conn, acc, s[l.sl])
    W[l.sl] = r['weights'].reshape(-1)
    new_mask = r['mask'].reshape(-1)
    mask[l.sl] = new_mask
    lifted = np.where(r['mask1'] == 1, F32(np.min(sg) - F32(1)), sg).astype(F32)
    counts.append([r['n_ones'], r['n_prune'], r['n_keep'], int(new_conn.sum()), 0,
                   _ties_admitted(sd, r['idx1'], r['n_keep']), _ties_admitted(lifted, r['idx2'], r['n_prune']),
                   int(new_mask.sum())])
    facts.append(dict(scope=l.scope, n_prune=r['n_prune'], grown=int(np.logical_and(new_mask == 1, m == 0).sum()),
                      reinit=int(np.logical_and(new_conn, m == 1).sum()), mask_changed=not np.array_equal(new_mask, m)))
  return W, mask, slots, np.array(counts, np.int32).reshape(-1, 8), facts


def topk_masks(arena, scores_of, sparsities):
  """so:302-316 / so:445-459: per layer, ones at the n_keep = n - get_n_zeros(n, s) largest scores, ties by lower index."""
  mask = np.zeros(arena.n_masked, F32)
  for l in arena.layers:
    n_keep = l.numel - O.get_n_zeros(l.numel, sparsities[l.mask_name])
    new = np.zeros(l.numel, F32)
    new[O.topk_order(scores_of(l))[:n_keep]] = 1
    mask[l.sl] = new
  return mask


# ------------------------------------------------------------------------------------------------ one optimizer call
def step(cfg, arena, st, G, rand=None, strict_rand=False, mutant=None):
  """One ``apply_gradients`` (after ``compute_gradients`` left ``G`` in the gradient arena).  Returns (state, info)."""
  assert mutant is None or mutant in MUTANTS
  G = np.asarray(G, F32)
  draw = _Draws(cfg, rand, strict_rand)
  new = dict(st)
  new['ema'] = dict(st['ema'])
  info = dict(is_update=False, drop_fraction=None, counts=None, facts=[], applied=False)
  if cfg.method in SET_FAMILY:
    _set_family(cfg, arena, st, G, draw, mutant, new, info)
  elif cfg.method == 'rigl':
    _rigl(cfg, arena, st, G, draw, mutant, new, info)
  elif cfg.method == 'snip':
    _snip(cfg, arena, st, G, mutant, new, info)
  else:
    _dnw(cfg, arena, st, G, mutant, new, info)
  info['draws'] = draw.log
  return new, info


def _gate(cfg, gs, last):
  is_upd = O.is_mask_update_iter(gs, last, cfg.begin, cfg.end, cfg.frequency)              # base:198-230
  return is_upd, O.get_drop_fraction(cfg.anneal, cfg.drop_fraction, gs, cfg.begin, cfg.end, is_upd)   # base:232-258


def _set_family(cfg, arena, st, G, draw, mutant, new, info):
  mask = st['mask']
  if cfg.method == 'snfs':                                       # base:133 -> so:195-197, before the apply
    omd = F32(1.0 - cfg.ema_decay)                               # ExponentialMovingAverage: decay = 1 - decay in python floats
    for l in arena.layers:
      e = st['ema'].get(l.name)
      e = np.zeros(l.numel, F32) if e is None else e
      g = G[l.sl]
      if mutant == 'ema_of_masked_gradient':
        g = (mask[l.sl] * g).astype(F32)
      new['ema'][l.name] = (e - ((e - g).astype(F32) * omd).astype(F32)).astype(F32)
  W, slots, bp = inner_apply(cfg, arena, st, G, _full_mask(arena, mask), arena.wd)          # base:134-136, every call
  gs = st['gs'] + 1
  new.update(W=W, slots=slots, beta_powers=bp, gs=gs)
  info['applied'] = True
  is_upd, frac = _gate(cfg, gs, st['last_update_step'])          # base:145-146 with the incremented step
  info.update(is_update=is_upd, drop_fraction=frac)
  if not is_upd:
    return
  W2, mask2, slots2, counts, facts = mask_update(
      cfg, arena, W, mask, slots, G, new['ema'], frac, gs - 1 if mutant == 'seed_step_before_increment' else gs, draw, mutant,
      W_scores=st['W'] if mutant == 'set_update_on_pre_apply_weights' else None,
      ema_scores=st['ema'] if mutant == 'ema_updated_after_the_update' else None)
  new.update(W=W2, mask=mask2, slots=slots2, last_update_step=gs)          # base:178-180
  info.update(counts=counts, facts=facts)


def _rigl(cfg, arena, st, G, draw, mutant, new, info):
  gs = st['gs']
  is_upd, frac = _gate(cfg, gs, st['last_update_step'])          # base:508-521: the cond's false branch is the apply
  info.update(is_update=is_upd, drop_fraction=frac)
  if is_upd:
    cur = st
    if mutant == 'rigl_applies_on_update_call':
      W, slots, bp = inner_apply(cfg, arena, st, G, _full_mask(arena, st['mask']), arena.wd)
      cur = dict(st, W=W, slots=slots)
      new.update(beta_powers=bp, gs=gs + 1)
    W2, mask2, slots2, counts, facts = mask_update(cfg, arena, cur['W'], st['mask'], cur['slots'], G, {}, frac, gs, draw, mutant)
    new.update(W=W2, mask=mask2, slots=slots2, last_update_step=gs)
    info.update(counts=counts, facts=facts)
    return
  W, slots, bp = inner_apply(cfg, arena, st, G, _full_mask(arena, st['mask']), arena.wd)
  new.update(W=W, slots=slots, beta_powers=bp, gs=gs + 1)
  info['applied'] = True


def _sparsities(cfg, arena):
  return O.get_sparsities(arena.mask_shapes(), cfg.mask_init_method, cfg.default_sparsity, cfg.custom_sparsity_map)


def _snip(cfg, arena, st, G, mutant, new, info):
  if st['gs'] == 0 and not st['is_snipped']:                     # so:332-335
    W, mask = st['W'], st['mask']

    def score(l):                                                # so:299-301: |g * v|, g w.r.t. the variable, l2 included
      wd = 0.0 if mutant == 'snip_score_without_wd' else arena.wd[l.sl]
      g = O.masked_grad(G[l.sl], mask[l.sl], W[l.sl], wd)
      return np.abs((g * W[l.sl]).astype(F32))

    new.update(mask=topk_masks(arena, score, _sparsities(cfg, arena)), is_snipped=True)
    if mutant == 'snip_increments_step':
      new['gs'] = st['gs'] + 1
    info['is_update'] = True
    info['facts'] = [dict(scope=l.scope, mask_changed=not np.array_equal(new['mask'][l.sl], mask[l.sl])) for l in arena.layers]
    return
  W, slots, bp = inner_apply(cfg, arena, st, G, _full_mask(arena, st['mask']), arena.wd)
  new.update(W=W, slots=slots, beta_powers=bp, gs=st['gs'] + 1)
  info['applied'] = True


def _dnw(cfg, arena, st, G, mutant, new, info):
  wd = arena.wd.copy()
  if mutant != 'dnw_l2_on_masked_kernels':
    wd[:arena.n_masked] = 0                                      # so:379-386: the regulariser does not reach mask*W
  if mutant == 'dnw_no_l2_on_dense_kernels':
    wd[arena.n_masked:arena.n_kernel] = 0
  m = _full_mask(arena, st['mask']) if mutant == 'dnw_masked_gradient' else np.ones(arena.total, F32)
  W, slots, bp = inner_apply(cfg, arena, st, G, m, wd)           # so:423-424
  shift = 1 if mutant == 'dnw_scores_shifted_by_one' else 0
  mask = topk_masks(arena, lambda l: np.abs(W[l.offset + shift:l.offset + shift + l.numel]), _sparsities(cfg, arena))   # so:444
  new.update(W=W, slots=slots, beta_powers=bp, gs=st['gs'] + 1, mask=mask)
  info.update(applied=True, is_update=True)
  info['facts'] = [dict(scope=l.scope, mask_changed=not np.array_equal(mask[l.sl], st['mask'][l.sl])) for l in arena.layers]


# ------------------------------------------------------------------------------------------------ comparing
def reduction_bound(n):
  """Relative bound on an fp32 mean |W| or population std of n values against its float64 value, whatever the order of the
  device's reduction: a sum of n non-negative fp32 terms carries at most (n - 1) roundings of relative size u = 2^-24 on any
  term's path, in any order; forming each term (|w|, or (w - mean)^2 with its subtraction and product), the division by
  n, the square root (which halves a relative error) and the final rounding add less than 8 more.  The std's mean is itself
  off by at most n u mean|W|, which enters the variance only squared.  So (n + 8) * 2^-24 holds for both.  On the layers
  of the tests (512 ... 235 200 weights) that is 3e-5 ... 1.4e-2; what it separates from the right value on the small layers
  of every case: Bessel's correction (1 / (2n) = 1e-3 at n = 512), a reduction over mask * W (a factor), over the padded
  slot (1000 -> 1024 weights: 2.4 %), over another layer's slice."""
  return (n + 8) * 2.0 ** -24


def compared(st, info):
  """Every array of a call's outcome that the tests compare, flat, in a fixed order (EMA tensors by name)."""
  arrs = [st['W'], st['mask'], np.array([len(st['slots'])])] + list(st['slots'])
  arrs.append(np.array([st['gs'], st['last_update_step'], int(st['is_snipped'])]))
  arrs.append(np.zeros(2, F32) if st['beta_powers'] is None else st['beta_powers'])
  arrs.append(np.array([len(st['ema'])]))
  arrs += [st['ema'][k] for k in sorted(st['ema'])]
  arrs.append(np.array([0 if info['drop_fraction'] is None else info['drop_fraction']], F32))
  arrs.append(np.zeros((0, 8), np.int32) if info['counts'] is None else info['counts'])
  return arrs


def outcomes_differ(a, ia, b, ib):
  ca, cb = compared(a, ia), compared(b, ib)
  return len(ca) != len(cb) or any(first_diff(x, y) is not None for x, y in zip(ca, cb))


def bf16_rne(x):
  """Round-to-nearest-even bfloat16 bits (uint16) of finite fp32 values."""
  u = np.asarray(x, F32).view(np.uint32).astype(np.uint64)
  return ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


def first_diff(a, b, nan_equal=False):
  """First flat index at which two arrays differ in a bit (None: none); fp32 is compared as uint32.  ``nan_equal``: a NaN on
  both sides counts as equal whatever its payload (x86's and gfx950's differ), as in adam_ref.same_bits."""
  a, b = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
  if a.shape != b.shape:
    return 0
  both_nan = None
  if nan_equal and a.dtype == np.float32 and b.dtype == np.float32:
    both_nan = np.isnan(a) & np.isnan(b)
  if a.dtype == np.float32:
    a = a.view(np.uint32)
  if b.dtype == np.float32:
    b = b.view(np.uint32)
  ne = a != b
  if both_nan is not None:
    ne &= ~both_nan
  d = np.flatnonzero(ne)
  return int(d[0]) if d.size else None
