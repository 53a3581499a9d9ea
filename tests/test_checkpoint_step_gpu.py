"""rigl_amd.checkpoint inside a training run.  The set-up of tests/test_accum_step_gpu.py::_replay_run: WRN depth 10, width 1, RigL
with period 5, ERK 0.8, droprate 0.3, a DeviceCifar over 64 images at batch 8, a device imagenet_lr_schedule, summaries attached.

  (a) 24 calls straight against 13 calls, save, everything dropped, a fresh graph / model / optimizer built from OTHER host seeds
      (weights and ERK masks), restore, 11 calls: W, slots, BITS, every moving statistic, the dropout counter, the DeviceCifar
      position, the global step, _last_update_step, the loss of each of the last 11 calls and the summaries records of those
      steps, bit for bit.  Mask updates run at calls 1, 7, 13, 19: call 13's lies directly in front of the save, and a second
      cut after call 12 puts it directly behind;
  (b) the same for eager -> eager, graph -> graph, eager -> graph, and Adam inside (beta powers);
  (c) SparseSETOptimizer at its default noise_std: the stateless draws carry no state;
  (d) SparseMomentumOptimizer (the gradient averages) and pruning.Pruning with a threshold update on each side of the save;
  (e) a rollback inside a live GraphedStep: same bits, the one graph kept, replays resumed, exactly one more eager step;
  (f) snapshot() followed at once by five more steps, then save: the file a fully synchronised save wrote in a twin run;
  (g) a TrainingState that is constructed and never used costs no launch and changes no bit;
  (h) refusals: a snapshot under capture, a snapshot with a MicroBatches sum pending, a WRN file into the MNIST MLP.
"""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BATCH = 8
CALLS, CUT = 24, 13


def _bits(t):
  return t.detach().cpu().numpy().reshape(-1).view(np.uint32).copy()


class _Run:
  """One training run: ``step()`` is one call of the loop."""

  def __init__(self, kind='rigl', optimizer='momentum', mode='eager', weight_seed=0, mask_seed=0, with_state=True):
    from rigl_amd import checkpoint, data, pruning, schedules as S, sparse_optimizers as SO, sparse_utils, summaries, train
    from rigl_amd import variables as V
    from rigl_amd.workloads import wide_resnet
    self.kind = kind
    sched = S.imagenet_lr_schedule(0.1, 32, num_train_images=40, model_architecture='mobilenet_v1')
    self.g = g = V.reset_default_graph(DEV)
    self.model = model = wide_resnet.WideResNet(g, depth=10, width=1, droprate=0.3, seed=weight_seed)
    if kind != 'prune':
      np.random.seed(mask_seed)
      sparse_utils.get_mask_init_fn(g.get_masks(), 'erdos_renyi_kernel', 0.8, {})()
    if optimizer == 'adam':
      self.inner = inner = train.AdamOptimizer(0.001, graph=g)
    else:
      self.inner = inner = train.MomentumOptimizer(sched, 0.9, use_nesterov=True, graph=g)
    self.pruner = None
    if kind == 'rigl':
      self.opt = SO.SparseRigLOptimizer(inner, 0, 1000, 5, drop_fraction=0.3, drop_fraction_anneal='cosine', noise_std=0.)
    elif kind == 'set':
      self.opt = SO.SparseSETOptimizer(inner, 0, 1000, 5, drop_fraction=0.3, drop_fraction_anneal='cosine')
    elif kind == 'snfs':
      self.opt = SO.SparseMomentumOptimizer(inner, 0, 1000, 5, drop_fraction=0.3, drop_fraction_anneal='cosine')
    else:
      self.opt = inner
    self.gs = gs = g.get_or_create_global_step()
    if kind == 'prune':
      # (every update of a threshold mixes in the one before: the thresholds are state)
      spec = pruning.get_pruning_hparams().parse('begin_pruning_step=0,pruning_frequency=4,threshold_decay=0.5,target_sparsity=0.6,'
                                                 'sparsity_function_begin_step=0,sparsity_function_end_step=20')
      self.pruner = pruning.Pruning(spec, gs, graph=g)
    rng = np.random.RandomState(11)
    images = rng.randint(0, 256, (64, 32, 32, 3)).astype(np.uint8)
    labels = rng.randint(0, 10, 64).astype(np.int32)
    self.dc = dc = data.DeviceCifar(images, labels, BATCH, seed=5, device=DEV)

    def loss_fn():
      x, y = dc.next_batch()
      return model.loss(x, y)
    self.loss_fn = loss_fn
    self.summ = summaries.TrainingSummaries(g, self.opt, ring=64).attach()
    self.st = train.GraphedStep(loss_fn, self.opt, gs, warmup=2) if mode == 'graph' else None
    self.state = checkpoint.TrainingState(g, self.opt, model=model, data=[dc], pruning=self.pruner,
                                          extra={'kind': kind}) if with_state else None
    self.losses = []

  def step(self):
    if self.st is not None:
      loss = self.st()
    else:
      loss = self.loss_fn()
      self.opt.minimize(loss, self.gs)
    if self.pruner is not None:
      self.pruner.conditional_mask_update_op()
    self.losses.append(float(loss.detach().float()))

  def steps(self, n):
    for _ in range(n):
      self.step()
    return self

  def final(self, records=True):
    from rigl_amd.workloads import nn as gnn
    torch.cuda.synchronize()
    g, inner = self.g, self.inner
    bns = [m for m in g.modules.values() if isinstance(m, gnn.BatchNorm)]
    out = dict(W=_bits(g.W), A=_bits(inner._slot), B=g.BITS.cpu().numpy().copy(), gs=int(self.gs.value),
               stats=[_bits(t) for b in bns for t in (b.moving_mean, b.moving_variance)],
               dropout=int(self.model.dropout_state.step.item()), position=self.dc.position(),
               last_update=getattr(self.opt, '_last_update_step', None), losses=list(self.losses))
    if getattr(inner, '_slot_v', None) is not None:
      out['V'], out['beta'] = _bits(inner._slot_v), _bits(inner._beta_powers)
    if self.kind == 'snfs':
      out['ema'] = [_bits(self.opt._ema[w.name]) for w in self.opt.get_weights()]
    if self.pruner is not None:
      out['thresholds'] = _bits(self.pruner._state.thresholds)
      out['prune_last'] = int(self.pruner._state.last_mask_update_step)
    if records:
      out['records'], out['dropped'] = self.summ.read(per_variable=True)
    return out


_CACHE = {}


def _straight(kind, optimizer, mode):
  key = (kind, optimizer, mode)
  if key not in _CACHE:
    _CACHE[key] = _Run(kind, optimizer, mode).steps(CALLS).final()
  return _CACHE[key]


def _interrupted(tmp_path, kind, optimizer, mode1, mode2, cut=CUT):
  path = str(tmp_path / 'ckpt')
  first = _Run(kind, optimizer, mode1).steps(cut)
  first.state.save(path)
  saved = first.final(records=False)
  del first
  second = _Run(kind, optimizer, mode2, weight_seed=7, mask_seed=3)
  before = second.final(records=False)
  assert not np.array_equal(before['W'], saved['W'])            # other weights ...
  if kind != 'prune':
    assert not np.array_equal(before['B'], saved['B'])          # ... and other masks
  assert second.state.restore(path) == {'kind': kind}
  restored = second.final(records=False)
  for key in ('W', 'A', 'B'):
    np.testing.assert_array_equal(restored[key], saved[key])
  second.steps(CALLS - cut)
  return saved, second.final(), second


def _compare(straight, resumed, cut=CUT):
  for key in ('W', 'A', 'B', 'V', 'beta', 'thresholds'):
    assert (key in straight) == (key in resumed)
    if key in straight:
      assert int(np.count_nonzero(straight[key] != resumed[key])) == 0, key
  assert len(straight['stats']) >= 10 and len(straight['stats']) == len(resumed['stats'])
  assert all(np.array_equal(x, y) for x, y in zip(straight['stats'], resumed['stats']))
  if 'ema' in straight:
    assert len(straight['ema']) == len(resumed['ema']) > 0
    assert all(np.array_equal(x, y) for x, y in zip(straight['ema'], resumed['ema']))
  for key in ('gs', 'dropout', 'position', 'last_update', 'prune_last'):
    assert straight.get(key) == resumed.get(key), key
  assert straight['dropout'] == straight['position'] == CALLS
  tail = straight['losses'][cut:]
  assert len(tail) == CALLS - cut == len(resumed['losses']) and all(np.isfinite(tail))
  assert tail == resumed['losses']
  assert straight['dropped'] == resumed['dropped'] == 0
  first_step = resumed['records'][0]['global_step']
  want = [r for r in straight['records'] if r['global_step'] >= first_step]
  assert len(want) == len(resumed['records']) >= 8 and want == resumed['records']


# ---- (a), (b) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('optimizer,mode1,mode2', [('momentum', 'eager', 'eager'), ('momentum', 'graph', 'graph'),
                                                   ('momentum', 'eager', 'graph'), ('adam', 'eager', 'eager')])
def test_ab_straight_against_interrupted(tmp_path, optimizer, mode1, mode2):
  straight = _straight('rigl', optimizer, mode2)
  saved, resumed, run = _interrupted(tmp_path, 'rigl', optimizer, mode1, mode2)
  # calls 1, 7, 13, 19 update the masks: the save after call 13 has one directly in front of it and one on each side
  assert saved['gs'] == 10 and saved['last_update'] == 10 and straight['gs'] == CALLS - 4 and straight['last_update'] == 15
  _compare(straight, resumed)
  assert not np.array_equal(saved['B'], resumed['B'])           # the masks moved behind the save
  if mode2 == 'graph':
    assert run.st.replays > 0 and len(run.st._graphs) == 1


def test_a_a_mask_update_directly_behind_the_save(tmp_path):
  straight = _straight('rigl', 'momentum', 'eager')
  saved, resumed, _ = _interrupted(tmp_path, 'rigl', 'momentum', 'eager', 'eager', cut=12)
  assert saved['gs'] == 10 and saved['last_update'] == 5        # the first call behind the restore is the update at step 10
  _compare(straight, resumed, cut=12)


# ---- (c), (d) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['set', 'snfs', 'prune'])
def test_cd_other_methods(tmp_path, kind):
  straight = _straight(kind, 'momentum', 'eager')
  saved, resumed, run = _interrupted(tmp_path, kind, 'momentum', 'eager', 'eager')
  if kind == 'set':
    assert run.opt._noise_std == 1e-5                           # the default: the drop scores carry noise drawn per (seed, step)
  if kind == 'snfs':
    assert any(n.startswith('snfs/ema/') for n in run.state.region_names())
  if kind == 'prune':
    # threshold updates at steps 4, 8, 12 | 16, 20, 24: on each side of the save (13 calls = 13 steps here)
    assert saved['gs'] == CUT and saved['prune_last'] == 12 and straight['prune_last'] == 24
    assert 'pruning/thresholds' in run.state.region_names() and np.count_nonzero(saved['thresholds']) > 0
    assert not np.array_equal(saved['thresholds'], straight['thresholds'])
    assert straight['gs'] == CALLS and straight['last_update'] is None
  else:
    # SET's family steps on every call and updates the masks behind the step: updates on each side of the save
    assert saved['gs'] == CUT and 0 < saved['last_update'] < straight['last_update'] and straight['last_update'] > CUT
  _compare(straight, resumed)


# ---- (e) ---------------------------------------------------------------------------------------------------------------------
def test_e_rollback_in_a_live_graphed_step():
  run = _Run('rigl', 'momentum', 'graph').steps(10)
  st = run.st
  snap = run.state.snapshot()
  e0, r0 = st.eager_steps, st.replays
  run.steps(10)
  first = run.final()
  e1, r1 = st.eager_steps, st.replays
  assert r1 > r0 > 0 and len(st._graphs) == 1
  graph_before = next(iter(st._graphs.values()))[0]
  run.state.restore(snap)
  assert int(run.gs.value) == 8 and run.opt._last_update_step == 5
  run.losses = run.losses[:10]
  run.steps(10)
  second = run.final()
  for key in ('W', 'A', 'B'):
    assert int(np.count_nonzero(first[key] != second[key])) == 0, key
  assert all(np.array_equal(x, y) for x, y in zip(first['stats'], second['stats']))
  for key in ('gs', 'dropout', 'position', 'last_update', 'losses'):
    assert first[key] == second[key], key
  assert [r for r in first['records'] if r['global_step'] >= 8] == second['records']
  assert len(st._graphs) == 1 and next(iter(st._graphs.values()))[0] is graph_before      # no recapture
  assert st.eager_steps - e1 == (e1 - e0) + 1                   # one eager step uploads the stale counters, then replays resume
  assert st.replays - r1 == (r1 - r0) - 1


# ---- (f) ---------------------------------------------------------------------------------------------------------------------
def test_f_snapshot_is_non_blocking_and_consistent(tmp_path):
  a = _Run('rigl', 'momentum', 'eager').steps(CUT)
  snap = a.state.snapshot()
  for _ in range(5):                                            # at once, nothing synchronised in between
    loss = a.loss_fn()
    a.opt.minimize(loss, a.gs)
  snap.save(str(tmp_path / 'a'))
  moved = _bits(a.g.W)
  del a
  b = _Run('rigl', 'momentum', 'eager').steps(CUT)
  torch.cuda.synchronize()
  b.state.save(str(tmp_path / 'b'))
  torch.cuda.synchronize()
  assert not np.array_equal(moved, _bits(b.g.W))                # the five steps did move the weights
  raw_a, raw_b = open(str(tmp_path / 'a'), 'rb').read(), open(str(tmp_path / 'b'), 'rb').read()
  assert len(raw_a) == len(raw_b) > 1 << 16 and raw_a == raw_b
  # a second snapshot reuses the one staging buffer and leaves the first one's image alone
  s1 = b.state.snapshot()
  b.steps(1)
  s2 = b.state.snapshot()
  assert s1.tobytes() == raw_b and s2.tobytes() != raw_b


# ---- (g) ---------------------------------------------------------------------------------------------------------------------
def test_g_free_when_unused():
  from rigl_amd import checkpoint, ops
  with_state = _Run('rigl', 'momentum', 'eager', with_state=True).steps(8).final()
  without = _Run('rigl', 'momentum', 'eager', with_state=False).steps(8).final()
  for key in ('W', 'A', 'B'):
    np.testing.assert_array_equal(with_state[key], without[key])
  assert with_state['losses'] == without['losses'] and with_state['records'] == without['records']
  counts = []
  for build in (False, True):
    run = _Run('rigl', 'momentum', 'eager', with_state=False).steps(3)        # buffers and code objects settle; step 2 comes next
    torch.cuda.synchronize()
    ops.prof_enable(True)
    try:
      ops.prof_collect()
      if build:
        state = checkpoint.TrainingState(run.g, run.opt, model=run.model, data=[run.dc])
        made = {k: v[1] for k, v in ops.prof_collect().items()}
        assert sum(made.values()) == 0, made                     # constructing one enqueues no launch
        assert state._staging is None and state._host is None    # ... and allocates nothing
      run.step()
      counts.append({k: v[1] for k, v in ops.prof_collect().items()})
    finally:
      ops.prof_enable(False)
  assert counts[0] == counts[1] and sum(counts[0].values()) > 10


# ---- (h) ---------------------------------------------------------------------------------------------------------------------
def test_h_refusals(tmp_path):
  from rigl_amd import checkpoint, train, variables as V
  from rigl_amd.workloads import mnist_mlp
  run = _Run('rigl', 'momentum', 'eager').steps(3)
  torch.cuda.synchronize()
  scratch = torch.zeros(8, device=DEV)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    scratch.add_(1.0)
    with pytest.raises(RuntimeError, match='capture'):
      run.state.snapshot()
    with pytest.raises(RuntimeError, match='capture'):
      run.state.restore(str(tmp_path / 'none'))
  torch.cuda.synchronize()
  # a MicroBatches sum pending
  mb = train.MicroBatches(run.loss_fn, run.opt, micro_batches=2)
  loss = mb()
  with pytest.raises(RuntimeError, match='pending'):
    run.state.snapshot()
  run.opt.minimize(loss, run.gs)
  path = str(tmp_path / 'wrn')
  run.state.save(path)                                          # the step is finished: fine again
  # a WRN file into the MNIST MLP
  g = V.reset_default_graph(DEV)
  mnist_mlp.MnistMLP(g)
  inner = train.MomentumOptimizer(0.1, 0.9, use_nesterov=True, graph=g)
  other = checkpoint.TrainingState(g, inner)
  w0 = _bits(g.W)
  with pytest.raises(checkpoint.CheckpointError, match='does not fit'):
    other.restore(path)
  torch.cuda.synchronize()
  np.testing.assert_array_equal(_bits(g.W), w0)
  assert int(g.get_or_create_global_step().value) == 0
