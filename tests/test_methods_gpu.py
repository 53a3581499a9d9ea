"""SET, Static, SNFS, RigL, SNIP and DNW steps on real nets, bit for bit against tests/method_ref.py.

Workloads: mnist_mlp.MnistMLP at batch 100 (three FC layers, layer3 at custom sparsity 0) and
wide_resnet.WideResNet(depth=22, width=1) at batch 16 (21 masked layers in padded arena slots, a dense stem, BN and bias
segments, l2 5e-4).  A case is 8 optimizer calls with a fresh synthetic batch per call.  Before each call the device's
state is copied to the host: W, G (after compute_gradients), the mask bitmap, the slot arenas and beta powers, the EMA
tensors, the global step, the last update step.  The random tensors the call draws are recorded by wrappers around
ops.stateless_random / ops.stateless_random_batched that clone the outputs; nothing in the product is replaced.  After the
call every arena segment of W, every slot, the beta powers, every bitmap word, every EMA tensor, the global step, the last
update step, the drop fraction, the update's counts and is_snipped must equal method_ref's bit for bit, and after
refresh_shadows() every layer's HWIO / OHWI shadow must be the round-to-nearest-even bf16 of mask * W.

The only tolerance is the one tests/test_tf_random.py already holds the normal stream to, atol = stddev * 2e-6 (ocml's
sinf / cosf / logf against glibc's): the normal tensors are the reference's input, and are held to the oracle's stream --
tag, step and all -- separately.  Uniform tensors are computed by the reference itself and compared bit for bit.  One
quantity is held at a derived bound and not bit for bit: the device's reductions mean |W| and std(W) behind grow_init
random_uniform_d / random_normal_d, whose order of summation is the device's (method_ref.reduction_bound).

Every case also asserts on what it ran that it has the property it is there for (updates happened, with training between
them; connections were pruned in two layers and grown where the mask was 0; Static re-initialised without changing a
mask; DNW changed a mask and moved masked-off weights; SNIP's l2 changed the kept set), and that its own data tells the
reference from every mutant order of operations of method_ref.MUTANTS that applies to it.  Two cases give the masked
kernels two different decays, which sends the inner optimizers through the per-variable update path."""
import time

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import method_ref as R  # noqa: E402
from oracle import tf_random as T  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
CALLS = 8
WRN = 'resnet_model/'


# ------------------------------------------------------------------------------------------------------------ the cases
def _case(method, inner, net, **kw):
  return dict(method=method, inner=inner, net=net, kw=kw)


def _id(c):
  extra = '-'.join('%s' % v for k, v in sorted(c['kw'].items()) if k in ('grow_init', 'initial_acc_scale', 'map'))
  if c['kw'].get('mixed_wd'):
    extra = (extra + '-mixedwd').lstrip('-')
  return '-'.join(x for x in (c['method'], c['inner'], c['net'], extra) if x)


CASES = []
for _m in ('set', 'static', 'snfs'):
  for _i in ('sgd', 'momentum', 'adam'):
    CASES.append(_case(_m, _i, 'mlp'))
CASES += [_case('set', 'momentum', 'wrn'), _case('static', 'adam', 'wrn'), _case('snfs', 'sgd', 'wrn')]
# initial_acc_scale = 0.5 goes with momentum.  With Adam, reset_momentum (base:555-564) assigns grad * initial_acc_scale to
# the second moment as well: it goes negative where the gradient is, the next ApplyAdam takes its square root, and from the
# forward pass behind that every value of the run is NaN -- in the reference and on the device alike -- so a second update
# would rank NaN scores, whose order tf.nn.top_k does not define.  The 8-call Adam cases therefore run with 0, and the three
# calls that carry the behaviour (apply, update, apply) are test_rigl_adam_initial_acc_scale_resets_both_slots_... below.
for _n, _gi in enumerate(('zeros', 'grad_scale_2', 'random_uniform_2', 'random_normal_2')):
  CASES.append(_case('rigl', 'momentum', 'mlp', grow_init=_gi, initial_acc_scale=0.5 if _n % 2 == 0 else 0.0))
  CASES.append(_case('rigl', 'adam', 'mlp', grow_init=_gi, initial_acc_scale=0.0))
CASES += [_case('rigl', 'momentum', 'wrn', grow_init='zeros', initial_acc_scale=0.5),
          _case('rigl', 'adam', 'wrn', grow_init='random_uniform_2', initial_acc_scale=0.0),
          _case('rigl', 'momentum', 'wrn', grow_init='random_normal_2', initial_acc_scale=0.0)]
CASES += [_case('snip', 'momentum', 'wrn', map=False), _case('snip', 'momentum', 'wrn', map=True),
          _case('snip', 'momentum', 'mlp', map=True)]
CASES += [_case('dnw', 'sgd', 'wrn', map=True), _case('dnw', 'momentum', 'wrn', map=True), _case('dnw', 'sgd', 'mlp', map=True)]
# two decays among the masked kernels: the inner optimizers then update variable by variable (train._apply_per_variable),
# where DNW's "no l2 on the masked kernels" and the others' per-layer decay are decided a second time
CASES += [_case('dnw', 'momentum', 'mlp', map=True, mixed_wd=True), _case('set', 'adam', 'mlp', mixed_wd=True)]

LR = {'sgd': 0.1, 'momentum': 0.05, 'adam': 1e-3}


def _sparsity_setup(c):
  """(mask_init_method, default_sparsity, custom_sparsity_map) of a case: one layer at 0.0 and one at 0.98 wherever a map is
  asked for; the dynamic methods start from the workloads' usual distributions (MLP: layer3 dense)."""
  if c['method'] in ('snip', 'dnw'):
    if not c['kw'].get('map'):
      return 'random', 0.5, {}
    if c['net'] == 'mlp':
      return 'random', 0.5, {'layer3': 0.0, 'layer2': 0.98}
    return 'erdos_renyi_kernel', 0.8, {WRN + 'logits': 0.0, WRN + 'conv_4_2_2': 0.98}
  return ('random', 0.9, {'layer3': 0.0}) if c['net'] == 'mlp' else ('erdos_renyi_kernel', 0.8, {})


def _build(c):
  from rigl_amd import sparse_optimizers as SO, sparse_utils, train, variables as V
  from rigl_amd.workloads import mnist_mlp, wide_resnet
  g = V.reset_default_graph(DEV)
  if c['net'] == 'mlp':
    model, batch, mod = mnist_mlp.MnistMLP(g), 100, mnist_mlp
  else:
    model, batch, mod = wide_resnet.WideResNet(g, depth=22, width=1), 16, wide_resnet
  if c['kw'].get('mixed_wd'):
    g.layers_by_scope['layer2'].weights.weight_decay = 3e-4
  init, s, cmap = _sparsity_setup(c)
  if c['method'] != 'snip':                       # SNIP starts dense (sparse_optimizers_test.py:404-410)
    np.random.seed(5)
    sparse_utils.get_mask_init_fn(g.get_masks(), init, s, cmap)()
  lr = LR[c['inner']]
  if c['inner'] == 'sgd':
    inner = train.GradientDescentOptimizer(lr, graph=g)
  elif c['inner'] == 'momentum':
    inner = train.MomentumOptimizer(lr, 0.9, use_nesterov=True, graph=g)
  else:
    inner = train.AdamOptimizer(lr, graph=g)
  cfg = R.Cfg(c['method'], c['inner'], lr=lr, mu=0.9, nesterov=True, default_sparsity=s, mask_init_method=init,
              custom_sparsity_map=cmap)
  m = c['method']
  if m in ('snip', 'dnw'):
    cls = SO.SparseSnipOptimizer if m == 'snip' else SO.SparseDNWOptimizer
    opt = cls(inner, s, init, custom_sparsity_map=cmap)
  else:
    # SET family: the step is incremented before the gate -> updates at calls 1, 4, 7.  RigL: an update call takes no step ->
    # updates at calls 1 and 5.  Either way at least two updates with training between them.
    cfg.begin, cfg.end, cfg.frequency = (1, 100, 3) if m == 'rigl' else (2, 100, 3)
    cfg.drop_fraction, cfg.anneal, cfg.noise_std, cfg.seed_offset = 0.3, 'cosine', 1e-5, 7
    kw = dict(drop_fraction=0.3, drop_fraction_anneal='cosine', stateless_seed_offset=7, noise_std=1e-5)
    if m == 'rigl':
      cfg.grow_init, cfg.initial_acc_scale = c['kw']['grow_init'], c['kw']['initial_acc_scale']
      kw.update(grow_init=cfg.grow_init, initial_acc_scale=cfg.initial_acc_scale)
    cls = {'set': SO.SparseSETOptimizer, 'static': SO.SparseStaticOptimizer, 'snfs': SO.SparseMomentumOptimizer,
           'rigl': SO.SparseRigLOptimizer}[m]
    opt = cls(inner, cfg.begin, cfg.end, cfg.frequency, **kw)
  return g, model, mod, batch, inner, opt, cfg


def _arena_of(g):
  """The arena layout and the per-element weight decay (each kernel's own, none on BN / biases) as method_ref wants them."""
  from rigl_amd import variables as V
  layers = []
  for l in g.masked_layers():
    layers.append(R.Layer(l.scope, l.weights.offset, l.weights.shape))
    assert layers[-1].name == l.weights.name and layers[-1].mask_name == l.mask.name
  total = g.W.numel()
  wd = np.zeros(total, F32)
  for v in g.trainable_variables():
    if v.kind in (V.KIND_MASKED, V.KIND_DENSE):
      wd[v.offset:v.offset + v.numel] = v.weight_decay
  assert g.seg[V.KIND_MASKED][0] == 0 and g.seg[V.KIND_DENSE][0] == g.seg[V.KIND_MASKED][1]
  return R.Arena(total, g.seg[V.KIND_MASKED][1], g.seg[V.KIND_DENSE][1], wd, layers)


# ------------------------------------------------------------------------------------------------------------ host copies
def _host(t):
  return t.detach().cpu().numpy().copy()


def _mask_of(g, arena):
  bits = _host(g.BITS).view(np.uint32)
  return np.unpackbits(bits.view(np.uint8), bitorder='little')[:arena.n_masked].astype(F32), bits


def _words(mask):
  return np.packbits(mask.astype(np.uint8), bitorder='little').view(np.uint32)


def _snapshot(g, arena, inner, opt, gs):
  inner._ensure_slots()                                        # the zero slots the first apply would create
  slots = tuple(_host(s) for s in (inner._slot, getattr(inner, '_slot_v', None)) if s is not None)
  bp = getattr(inner, '_beta_powers', None)
  return dict(W=_host(g.W), mask=_mask_of(g, arena)[0], slots=slots, beta_powers=None if bp is None else _host(bp),
              ema={k: _host(v).reshape(-1) for k, v in getattr(opt, '_ema', {}).items()}, gs=int(gs.value),
              last_update_step=int(getattr(opt, '_last_update_step', 0)), is_snipped=bool(getattr(opt, 'is_snipped', False)))


def _i32(v):
  v = int(v) & 0xFFFFFFFF
  return v - (1 << 32) if v >= 1 << 31 else v


class _Recorder:
  """Wraps the two entry points every random tensor of an optimizer call comes from; keeps a clone of each output."""

  def __init__(self, monkeypatch):
    from rigl_amd import ops
    self.records = []
    one, many = ops.stateless_random, ops.stateless_random_batched

    def stateless_random(n, seed0, seed1, dist, scale=1.0, shift=0.0, device=None, out=None):
      t = one(n, seed0, seed1, dist, scale=scale, shift=shift, device=device, out=out)
      self._keep(seed0, seed1, dist, scale, shift, t)
      return t

    def stateless_random_batched(items, device):
      outs = many(items, device)
      for (_, s0, s1, dist, scale, shift), t in zip(items, outs):
        self._keep(s0, s1, dist, scale, shift, t)
      return outs

    monkeypatch.setattr(ops, 'stateless_random', stateless_random)
    monkeypatch.setattr(ops, 'stateless_random_batched', stateless_random_batched)

  def _keep(self, s0, s1, dist, scale, shift, t):
    self.records.append(((_i32(s0), _i32(s1), dist), dict(scale=float(scale), shift=float(shift), out=t.clone())))

  def take(self):
    recs, self.records = self.records, []
    return {k: dict(v, out=_host(v['out']).reshape(-1)) for k, v in recs}


# ------------------------------------------------------------------------------------------------------------ comparing
def _where(arena, g, flat):
  """The variable an arena index belongs to (a masked layer's scope, another variable's name, or padding)."""
  for v in g.trainable_variables():
    if v.offset <= flat < v.offset + v.numel:
      return v.name
  return 'padding'


def _same(what, array, dev, ref, locate=None, nan_equal=False):
  """``nan_equal``: for the one test whose reference result holds NaNs (their payloads are the platform's)."""
  i = R.first_diff(dev, ref, nan_equal=nan_equal)
  if i is not None:
    d, r = np.asarray(dev).reshape(-1), np.asarray(ref).reshape(-1)
    pytest.fail('%s: %s differs, %s first at flat index %d (device %r, reference %r)'
                % (what, array, ('in %s, ' % locate(i)) if locate else '', i, d[i] if i < d.size else None, r[i] if i < r.size else None))


def _check_draws(what, cfg, info, rand):
  """The device drew exactly the tensors the reference asks for -- same tag, same step -- and they are the oracle's streams."""
  want = {d['seed'] + (d['dist'],): d for d in info['draws']}
  extra = set(rand) - set(want)
  assert not extra, '%s: the device drew tensors the reference has no use for, seeds %s' % (what, sorted(extra)[:3])
  for key, d in want.items():
    rec = rand[key]                                            # (present: the reference ran with strict_rand)
    tag = '%s %s/%s' % (what, d['layer'], d['tag'])
    assert rec['out'].size == d['n'], tag
    if d['tag'] == 'drop':
      assert (rec['scale'], rec['shift']) == (float(cfg.noise_std), 0.0), tag
    if d['tag'] == 'grow':
      assert (rec['scale'], rec['shift']) == (1.0, 0.0), tag
    # the two reductions of the device (base:382, :390): held to their float64 value of the weights the update saw at
    # method_ref.reduction_bound(n), a bound from the fp32 format alone -- the one quantity here that is not held bit for bit
    bound = R.reduction_bound(d['n'])
    if d['tag'] == 'grow_init_u':                              # minval = -mean |W|, maxval = mean |W|, maxval - minval in fp32
      assert rec['shift'] < 0 and F32(rec['scale']) == F32(-rec['shift']) - F32(rec['shift']), tag
      print('methods-reduction: %s mean|W| device %.9g float64 %.9g bound %.3g' % (tag, -rec['shift'], d['expect'], bound))
      assert abs(-rec['shift'] - d['expect']) <= bound * d['expect'], (tag, -rec['shift'], d['expect'], bound)
    if d['tag'] == 'grow_init_n':                              # stddev = reduce_std(W), the population's
      assert rec['shift'] == 0.0, tag
      print('methods-reduction: %s std(W) device %.9g float64 %.9g bound %.3g' % (tag, rec['scale'], d['expect'], bound))
      assert abs(rec['scale'] - d['expect']) <= bound * d['expect'], (tag, rec['scale'], d['expect'], bound)
    if d['dist'] == 'uniform':
      _same(tag, 'uniform tensor', rec['out'], d['value'])
    else:
      s0, s1 = d['seed']
      np.testing.assert_allclose(rec['out'], T.stateless_random_normal(d['n'], s0, s1, 0.0, rec['scale']), rtol=0,
                                 atol=rec['scale'] * 2e-6, err_msg=tag)


def _check_shadows(what, g, arena, new):
  """variables.py: hwio[i] = bf16(mask_i ? W_i : 0) in the weights' flat HWIO order, ohwi its [cout][kh*kw*cin] transpose."""
  g.refresh_shadows()
  for l in g.layers:
    o, n = l.weights.offset, l.weights.numel
    w = new['W'][o:o + n]
    if l.mask is not None:
      w = np.where(new['mask'][o:o + n] != 0, w, F32(0))
    hwio = R.bf16_rne(w)
    _same('%s %s' % (what, l.scope), 'HWIO shadow', _host(l.hwio.view(torch.int16)).view(np.uint16), hwio)
    _same('%s %s' % (what, l.scope), 'OHWI shadow', _host(l.ohwi.view(torch.int16)).view(np.uint16),
          hwio.reshape(l.k, l.cout).T.reshape(-1))


def _compare(what, g, arena, inner, opt, gs, cfg, new, info, nan_equal=False):
  from rigl_amd import variables as V
  locate = lambda i: _where(arena, g, i)                       # noqa: E731
  W = _host(g.W)
  for kind, name in ((V.KIND_MASKED, 'masked'), (V.KIND_DENSE, 'dense'), (V.KIND_OTHER, 'other')):
    b, e = g.seg[kind]
    _same(what, 'W (%s segment)' % name, W[b:e], new['W'][b:e], lambda i, b=b: _where(arena, g, b + i), nan_equal)
  for i, (s, nm) in enumerate(zip((inner._slot, getattr(inner, '_slot_v', None)), inner.get_slot_names())):
    _same(what, 'slot %r' % nm, _host(s), new['slots'][i], locate, nan_equal)
  if new['beta_powers'] is not None:
    _same(what, 'beta powers', _host(inner._beta_powers), new['beta_powers'])
  _same(what, 'mask bitmap (word index)', _mask_of(g, arena)[1], _words(new['mask']), lambda i: _where(arena, g, 32 * i))
  ema = getattr(opt, '_ema', {})
  assert sorted(ema) == sorted(new['ema']), what
  for l in arena.layers:
    if l.name in ema:
      _same('%s %s' % (what, l.scope), 'EMA', _host(ema[l.name]), new['ema'][l.name])
  assert int(gs.value) == new['gs'], '%s: global step %d, reference %d' % (what, gs.value, new['gs'])
  if hasattr(opt, '_last_update_step'):
    assert int(opt._last_update_step) == new['last_update_step'], '%s: last update step' % what
    _same(what, 'drop fraction', np.array([np.float32(opt.drop_fraction)]), np.array([info['drop_fraction']], F32))
    if info['counts'] is not None:
      _same(what, 'update counts [layer, 8]', _host(opt.last_counts), info['counts'], lambda i: arena.layers[i // 8].scope)
  if hasattr(opt, 'is_snipped'):
    assert bool(opt.is_snipped) == new['is_snipped'], '%s: is_snipped' % what


def _mutants_for(case, cfg):
  """The mutant references (method_ref.MUTANTS) that apply to a case.  Each must differ from the reference on the inputs the
  case actually ran: the device's data, not only the synthetic cases of test_method_ref_cpu.py, tell the orders apart."""
  m = cfg.method
  if m == 'set':
    out = ['set_update_on_pre_apply_weights', 'seed_step_before_increment', 'grow_drop_tags_swapped']
    out += ['rigl_momentum_reset_in_set'] if cfg.n_slots() else []
    return out + (['second_adam_slot_not_reset'] if cfg.inner == 'adam' else [])
  if m == 'static':
    return ['static_without_reinit']
  if m == 'snfs':
    return ['signed_ema_grow_score', 'ema_updated_after_the_update', 'ema_of_masked_gradient']
  if m == 'rigl':
    return ['rigl_applies_on_update_call', 'drop_noise_left_out']
  if m == 'snip':
    return ['snip_score_without_wd', 'snip_increments_step']
  out = ['dnw_l2_on_masked_kernels', 'dnw_masked_gradient', 'dnw_scores_shifted_by_one']
  return out + (['dnw_no_l2_on_dense_kernels'] if case['net'] == 'wrn' else [])     # (the MLP has no dense kernel)


# ------------------------------------------------------------------------------------------------------------ the test
def _run(case, monkeypatch, calls, mutants=False, nan_equal=False):
  """``calls`` optimizer calls of a case, each compared with the reference.  Returns what the case did."""
  g, model, mod, batch, inner, opt, cfg = _build(case)
  arena = _arena_of(g)
  gs = g.get_or_create_global_step()
  rec = _Recorder(monkeypatch)
  did = dict(cfg=cfg, gs=gs, updates=[], facts=[], moved=0, changed=False, snip_differs=None, calls=[])
  did['untold'] = _mutants_for(case, cfg) if mutants else []
  for call in range(calls):
    what = '%s call %d' % (_id(case), call)
    x, y = mod.synthetic_batch(batch, DEV, seed=1000 + call)
    gv = opt.compute_gradients(model.loss(x, y))
    st = _snapshot(g, arena, inner, opt, gs)
    G = _host(g.G)
    rec.take()
    opt.apply_gradients(gv, gs)
    rand = rec.take()
    new, info = R.step(cfg, arena, st, G, rand=rand, strict_rand=True)
    _check_draws(what, cfg, info, rand)
    _compare(what, g, arena, inner, opt, gs, cfg, new, info, nan_equal)
    if np.isfinite(new['W']).all():                            # (bf16_rne is for finite values)
      _check_shadows(what, g, arena, new)
    for mu in list(did['untold']):
      other, oinfo = R.step(cfg, arena, st, G, rand=rand, mutant=mu)
      if R.outcomes_differ(new, info, other, oinfo):
        did['untold'].remove(mu)
    if info['is_update']:
      did['updates'].append(call)
      did['facts'].append(info['facts'])
    if cfg.method == 'dnw':
      off = st['mask'] == 0
      did['moved'] += int((st['W'][:arena.n_masked][off] != new['W'][:arena.n_masked][off]).sum())
      did['changed'] |= any(f['mask_changed'] for f in info['facts'])
    if cfg.method == 'snip' and call == 0:
      other, _ = R.step(cfg, arena, st, G, mutant='snip_score_without_wd')
      did['snip_differs'] = not np.array_equal(other['mask'], new['mask'])
    did['calls'].append((st, new, info))
  torch.cuda.synchronize()
  return did


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_method_steps_match_the_reference(case, monkeypatch):
  t0 = time.time()
  did = _run(case, monkeypatch, CALLS, mutants=True)
  cfg, updates, facts_of = did['cfg'], did['updates'], did['facts']
  # ---- the case did what it is there for
  grown = sum(f.get('grown', 0) for fs in facts_of for f in fs)
  reinit = sum(f.get('reinit', 0) for fs in facts_of for f in fs)
  if cfg.method in R.SET_FAMILY + ('rigl',):
    assert len(updates) >= 2 and any(b - a > 1 for a, b in zip(updates, updates[1:])), updates
    for fs in facts_of:
      assert sum(f['n_prune'] >= 1 for f in fs) >= 2
      if cfg.method == 'static':
        assert sum(f['reinit'] for f in fs) >= 1 and not any(f['mask_changed'] for f in fs)
      else:
        assert sum(f['grown'] for f in fs) >= 1
  elif cfg.method == 'dnw':
    assert updates == list(range(CALLS)) and did['changed'] and did['moved'] > 0
  else:
    assert updates == [0] and did['snip_differs'] and int(did['gs'].value) == CALLS - 1
  assert not did['untold'], 'this run does not tell the reference from its mutants %s' % did['untold']
  print('\nmethods: %s %s %s %s updates=%d grown=%d reinit=%d seconds=%.2f'
        % (cfg.method, cfg.inner, case['net'], _id(case), len(updates), grown, reinit, time.time() - t0))


def test_rigl_adam_initial_acc_scale_resets_both_slots_like_the_reference(monkeypatch):
  """reset_momentum (base:555-564) assigns grad * initial_acc_scale to EVERY slot of a new connection, Adam's second moment
  included: where the gradient is negative ``v`` becomes negative, and the next ApplyAdam takes sqrt(v) -- NaN.  The device
  does what the reference does: after the update call both slots hold the same bits, negative ``v`` included, and after the
  next apply the weights are NaN at the same positions and equal in every other bit (a NaN's payload is the platform's, so
  NaN compares as NaN here and only here, as in adam_ref.same_bits).  Three calls: apply, update, apply."""
  case = _case('rigl', 'adam', 'mlp', grow_init='zeros', initial_acc_scale=0.5)
  with np.errstate(invalid='ignore'):
    did = _run(case, monkeypatch, 3, nan_equal=True)
  assert did['updates'] == [1]
  st, new, _ = did['calls'][1]                                 # the update call: no NaN yet, so every bit was compared
  n = st['mask'].size
  born = np.logical_and(st['mask'] == 0, new['mask'] == 1)
  m, v = new['slots'][0][:n], new['slots'][1][:n]
  assert np.isfinite(new['W']).all() and np.isfinite(v).all()
  assert born.sum() >= 1 and (v[born] < 0).sum() >= 1 and R.first_diff(v[born], m[born]) is None
  st, new, _ = did['calls'][2]                                 # the apply behind it
  assert np.array_equal(np.isnan(new['W'][:n]), np.logical_and(born, st['slots'][1][:n] < 0))
