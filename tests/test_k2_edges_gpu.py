"""K2 (prune_regrow.hip) at its edges, bit for bit against oracle.rigl_mask_update / get_update / topk_order (and
tests/prune_ref.py for the magnitude prune): every size of tests/k23_cases.py at every operand alignment, the degenerate
selection modes and the data edges (singly and inside batched calls), a 5000-layer table whose chunk ranges hold
complete, several and zero-length layers, the lifted-score overlap flag, and run-to-run identity.  Every operand that a
kernel writes or whose neighbourhood it could read wrongly lives between guard bands (k23_cases.Placement)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import k23_cases as K  # noqa: E402
import prune_ref as PR  # noqa: E402
from oracle import rigl_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
_TDT = {np.dtype(np.float32): torch.float32, np.dtype(np.uint32): torch.int32, np.dtype(np.uint16): torch.bfloat16}


def _bits(a):
  return np.ascontiguousarray(a, F32).reshape(-1).view(np.uint32)


def _same(name, got, ref):
  got, ref = _bits(got), _bits(ref)
  bad = np.nonzero(got != ref)[0]
  assert bad.size == 0, '%s: %d/%d differ, first at %s: got %s ref %s' % (
      name, bad.size, got.size, bad[:6], got[bad[:6]].view(F32), ref[bad[:6]].view(F32))


class Dev:
  """A Placement on the GPU: the image uploaded once, operands as tensor views into it."""

  def __init__(self, P):
    self.P = P
    self.buf = torch.from_numpy(P.buffer.copy()).to(DEV)

  def t(self, name):
    s, nb, dt = self.P.span(name)
    return self.buf[s:s + nb].view(_TDT[np.dtype(dt)])

  def ptr(self, name):
    return self.buf.data_ptr() + self.P.span(name)[0]

  def host(self):
    torch.cuda.synchronize()
    return self.buf.cpu().numpy()


def _grow_mode(c):
  from rigl_amd import _lib
  if c['grow_init'].startswith('grad_scale'):
    return _lib.GROW_GRAD_SCALE, O.extract_number(c['grow_init'])
  if c['grow_init'].startswith('grad_sign'):
    return _lib.GROW_GRAD_SIGN, O.extract_number(c['grow_init'])
  return _lib.GROW_ZEROS, 1.0


_OPERANDS = (('w', 'w'), ('g', 'dense_grad'), ('noise', 'drop_noise'), ('mom', 'momentum'), ('mom2', 'momentum2'))


def _place(cases, off):
  """All operands of some cases in one guarded buffer; returns (Dev, [layer dict per case])."""
  spec = {}
  for i, c in enumerate(cases):
    spec['bits%d' % i] = K.pack_bits(c['mask'])
    for key, _ in _OPERANDS:
      if c[key] is not None:
        spec['%s%d' % (key, i)] = c[key]
  D = Dev(K.Placement(spec, off))
  layers = []
  for i, c in enumerate(cases):
    l = dict(mask_bits=D.t('bits%d' % i))
    for key, arg in _OPERANDS:
      if c[key] is not None:
        l[arg] = D.t('%s%d' % (key, i))
    layers.append(l)
  return D, layers


def _results(D, cases, counts):
  host = D.host()
  assert D.P.guards_intact(host), 'a guard band was written'
  v = D.P.views(host)
  out = []
  for i, c in enumerate(cases):
    r = dict(mask=K.unpack_bits(v['bits%d' % i], c['mask'].size), bits=v['bits%d' % i].copy(), counts=counts[i])
    for key in ('w', 'mom', 'mom2', 'g', 'noise'):
      r[key] = v['%s%d' % (key, i)].copy() if c[key] is not None else None
    out.append(r)
  return out


def _run(cases, off, frac=None, selections=False):
  """prune_regrow on the cases as ONE call (their shared parameters are the first case's, `frac` overrides)."""
  from rigl_amd import ops
  c0 = cases[0]
  D, layers = _place(cases, off)
  mode, div = _grow_mode(c0)
  kw = dict(grow_init_mode=mode, grow_init_div=div, initial_acc_scale=c0['acc_scale'])
  frac = c0['frac'] if frac is None else frac
  if selections:
    sel = ops.prune_regrow_selections(layers[0], frac, **kw)
    counts = sel['counts'].cpu().numpy().reshape(1, -1)
  else:
    sel = None
    counts = ops.prune_regrow(layers, frac, **kw).cpu().numpy()
  res = _results(D, cases, counts)
  if sel is not None:
    n = c0['mask'].size
    res[0]['mask1'] = K.unpack_bits(sel['mask1_bits'].cpu().numpy().view(np.uint32), n)
    res[0]['mask2'] = K.unpack_bits(sel['mask2_bits'].cpu().numpy().view(np.uint32), n)
    res[0]['idx1'], res[0]['idx2'] = sel['idx1'].cpu().numpy(), sel['idx2'].cpu().numpy()
  return res


def _ties_admitted(score, idx, k):
  """out_counts[5] / [6]: how many of the k selected entries carry the threshold's score (0 when nothing is selected,
  n when everything is)."""
  n = score.size
  if k <= 0 or n == 0:
    return 0
  if k >= n:
    return n
  return int((score[idx[:k]] == score[idx[k - 1]]).sum())


_REF = {}


def _oracle(c):
  """The oracle's update of a case, computed once per case name and never modified."""
  key = (c['name'], c['frac'], c['grow_init'], c['acc_scale'])
  if key not in _REF:
    r = K.oracle_update(c) if c['mask'].size else None
    if r is not None:
      sd, sg = O.rigl_scores(c['mask'], c['w'], c['g'], c['noise'])
      with np.errstate(all='ignore'):
        lifted = np.where(r['mask1'] == 1, F32(sg.min() - F32(1)), sg).astype(F32)
      r['ties1'] = _ties_admitted(sd, r['idx1'], r['n_keep'])
      r['ties2'] = _ties_admitted(lifted, r['idx2'], r['n_prune'])
      if c['mom2'] is not None:
        r['momentum2'] = K.oracle_second_slot(c, r)
    _REF[key] = r
  return _REF[key]


def _check(c, got, what=''):
  """One layer's result against the oracle: masks, weights, slots and all eight counts; inputs untouched."""
  name = '%s %s' % (c['name'], what)
  cnt = got['counts']
  if c['mask'].size == 0:
    assert not cnt.any(), name
    return
  ones, prune, keep = K.expected_counts(c)
  assert (cnt[0], cnt[1], cnt[2]) == (ones, prune, keep), (name, cnt)
  r = _oracle(c)
  if r is None:                       # the reference's Assert fires: the flag says so, nothing else is promised
    assert cnt[4] != 0, name + ': overlap not reported'
    return
  assert cnt[4] == 0, name + ': overlap reported'
  _same(name + ' mask', got['mask'], r['mask'])
  np.testing.assert_array_equal(got['bits'], K.pack_bits(r['mask']), err_msg=name + ' bitmap words (tail bits zero)')
  _same(name + ' w', got['w'], r['weights'])
  if c['mom'] is not None:
    _same(name + ' momentum', got['mom'], r['momentum'])
  if c['mom2'] is not None:
    _same(name + ' momentum2', got['mom2'], r['momentum2'])
  _same(name + ' dense_grad (read only)', got['g'], c['g'])
  if c['noise'] is not None:
    _same(name + ' noise (read only)', got['noise'], c['noise'])
  assert cnt[3] == int(r['new_connections'].sum()), (name, cnt)
  assert cnt[5] == r['ties1'] and cnt[6] == r['ties2'], (name, cnt, r['ties1'], r['ties2'])
  assert cnt[7] == int(r['mask'].sum()), (name, cnt)
  if 'idx1' in got:
    _same(name + ' mask1', got['mask1'], r['mask1'])
    _same(name + ' mask2', got['mask2'], r['mask2'])
    np.testing.assert_array_equal(got['idx1'], r['idx1'], err_msg=name + ' idx1')
    np.testing.assert_array_equal(got['idx2'][:r['n_prune']], r['idx2'][:r['n_prune']], err_msg=name + ' idx2')


# ---- sizes x offsets x noise x slots -----------------------------------------------------------------------------------
@pytest.mark.parametrize('n', K.SIZES)
def test_every_size_offset_noise_and_slot_count(n):
  for noise in (False, True):
    for slots in (1, 2, 0):
      c = K.size_case(n, noise, slots)
      for off in K.OFFSETS:
        _check(c, _run([c], off)[0], 'off=%d' % off)
        _check(c, _run([c], off, selections=True)[0], 'off=%d selections' % off)


@pytest.mark.parametrize('n', K.SIZES)
def test_topk_mask_and_magnitude_prune_at_every_size_and_offset(n):
  from rigl_amd import ops
  s = K.score_case(n)
  w = K.size_case(n, True, 0)['w']
  old = (np.arange(n) % 3 == 0).astype(F32)
  for off in K.OFFSETS:
    for k in sorted({0, 1, n, K.zero_straddle_k(s) or 1}):
      D = Dev(K.Placement(dict(score=s, bits=np.full((n + 31) // 32, 0xFFFFFFFF, np.uint32)), off))
      ops.topk_mask(D.t('score'), k, out=D.t('bits'))
      host = D.host()
      assert D.P.guards_intact(host), 'topk_mask n=%d off=%d k=%d: guard hit' % (n, off, k)
      v = D.P.views(host)
      np.testing.assert_array_equal(v['bits'], K.pack_bits(K.topk_mask_ref(s, k)), err_msg='topk n=%d off=%d k=%d' % (n, off, k))
      _same('score (read only)', v['score'], s)
    for k in sorted({1, n}):
      for thr0, decay in ((0.0, 0.0), (0.125, 0.25)):
        D = Dev(K.Placement(dict(w=w, bits=K.pack_bits(old), thr=np.array([thr0], F32), counts=np.zeros(4, np.uint32)), off,
                            offsets=dict(thr=0)))
        ops.magnitude_prune_batched([(D.t('w'), D.t('bits'), D.t('thr'), k)], decay, counts=D.t('counts'))
        host = D.host()
        what = 'magnitude prune n=%d off=%d k=%d decay=%g' % (n, off, k, decay)
        assert D.P.guards_intact(host), what + ': guard hit'
        v = D.P.views(host)
        thr, m = PR.mask_update(w, k, thr0, decay)
        assert v['thr'].view(np.uint32)[0] == np.array([thr], F32).view(np.uint32)[0], what
        np.testing.assert_array_equal(v['bits'], PR.pack_bits(m), err_msg=what)
        assert v['counts'].tolist() == [n, k, int(m.sum()), int(old.sum())], what
        _same(what + ' w (read only)', v['w'], w)


@pytest.mark.parametrize('n', [33, 1025, 4097])
def test_explicit_scores_with_signed_zeros_and_infinities(n):
  """score_drop / score_grow given (the SET / Static path), -0.0 and +0.0 at the drop threshold: against oracle.get_update."""
  from rigl_amd import ops
  for c in K.explicit_score_cases(n):
    r = K.oracle_update_explicit(c)
    for off in K.OFFSETS:
      D = Dev(K.Placement(dict(w=c['w'], g=c['g'], mom=c['mom'], sd=c['score_drop'], sg=c['score_grow'], bits=K.pack_bits(c['mask'])), off))
      counts = ops.prune_regrow([dict(w=D.t('w'), dense_grad=D.t('g'), momentum=D.t('mom'), score_drop=D.t('sd'), score_grow=D.t('sg'),
                                      mask_bits=D.t('bits'))], c['frac'], initial_acc_scale=c['acc_scale']).cpu().numpy()[0]
      host = D.host()
      what = '%s off=%d' % (c['name'], off)
      assert D.P.guards_intact(host), what
      v = D.P.views(host)
      np.testing.assert_array_equal(v['bits'], K.pack_bits(r['mask']), err_msg=what)
      _same(what + ' w', v['w'], r['weights'])
      _same(what + ' momentum', v['mom'], r['momentum'])
      assert counts[:5].tolist() == [r['n_ones'], r['n_prune'], r['n_keep'], int(r['new_connections'].sum()), 0], (what, counts)
      assert counts[5] == _ties_admitted(c['score_drop'], r['idx1'], r['n_keep']) and counts[7] == int(r['mask'].sum()), (what, counts)


# ---- modes and data edges ----------------------------------------------------------------------------------------------
_SINGLE = {}


def _single(c):
  """The single-call result of a case at an unaligned base (computed once)."""
  if c['name'] not in _SINGLE:
    _SINGLE[c['name']] = _run([c], 1)[0]
  return _SINGLE[c['name']]


@pytest.mark.parametrize('c', K.all_k2_cases(), ids=lambda c: c['name'])
def test_mode_and_data_cases_singly(c):
  _check(c, _single(c))
  for off in (0, 3):
    _check(c, _run([c], off, selections=True)[0], 'off=%d selections' % off)
  assert int(_single(c)['counts'][4] != 0) == int(c['name'] == 'overlap')          # raised exactly on the overlap case


def _groups():
  g = {}
  for c in K.all_k2_cases():
    g.setdefault((c['frac'], c['grow_init'], c['acc_scale']), []).append(c)
  return list(g.values())


@pytest.mark.parametrize('group', _groups(), ids=lambda g: '+'.join(c['name'] for c in g))
def test_mode_and_data_cases_inside_a_batched_call(group):
  """Cases that share (drop_fraction, grow_init, initial_acc_scale) in ONE call between ordinary layers (one of them
  multi-chunk) and a zero-length one: a batched layer's result is its single-call result and the oracle's."""
  p = dict(frac=group[0]['frac'], grow_init=group[0]['grow_init'], acc_scale=group[0]['acc_scale'])
  ordinary = [dict(K.size_case(n, noise, 1, seed=9), name='ordinary%d' % n, **p) for n, noise in ((33, True), (8193, False), (1025, True))]
  empty = dict(K.size_case(0, False, 1), name='empty', **p)
  cases = [ordinary[0]]
  for c in group:
    cases += [c, ordinary[1 + len(cases) % 2]]
  cases.insert(len(cases) // 2, empty)
  res = _run(cases, 2)
  for c, got in zip(cases, res):
    _check(c, got, 'batched')
    if c['name'] in {x['name'] for x in group} and _oracle(c) is not None:
      one = _single(c)
      for key in ('bits', 'w', 'mom'):
        np.testing.assert_array_equal(got[key].view(np.uint32), one[key].view(np.uint32), err_msg='%s %s: batched != single' % (c['name'], key))
      assert got['counts'].tolist() == one['counts'].tolist(), c['name']
    assert int(got['counts'][4] != 0) == int(c['name'] == 'overlap'), c['name']


# ---- the 5000-layer table ----------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def table():
  t = K.table_case(K.layer_table())
  t['ref'] = [_oracle(K.table_layer(t, l)) for l in range(len(t['sizes']))]
  return t


def _table_dev(t, extra=None):
  spec = dict(w=t['w'], g=t['g'], mom=t['mom'], score=t['score'],
              bits=np.concatenate([K.pack_bits(t['mask'][int(a):int(b)]) for a, b in zip(t['start'], t['start'][1:])]))
  spec.update(extra or {})
  return Dev(K.Placement(spec, 1))


def test_layer_table_prune_regrow_every_layer_and_repeat_run(table):
  from rigl_amd import ops
  t = table
  nl = len(t['sizes'])
  images = []
  for _ in range(2):
    D = _table_dev(t)
    tw, tg, tm, tb = D.t('w'), D.t('g'), D.t('mom'), D.t('bits')
    layers = []
    for l in range(nl):
      a, b, wa, wb = int(t['start'][l]), int(t['start'][l + 1]), int(t['wstart'][l]), int(t['wstart'][l + 1])
      layers.append(dict(w=tw[a:b], dense_grad=tg[a:b], momentum=tm[a:b], mask_bits=tb[wa:wb]))
    counts = ops.prune_regrow(layers, t['frac'], initial_acc_scale=t['acc_scale']).cpu().numpy()
    host = D.host()
    assert D.P.guards_intact(host)
    images.append((host, counts))
  assert np.array_equal(images[0][0], images[1][0]) and np.array_equal(images[0][1], images[1][1]), 'two runs differ'
  v = D.P.views(images[0][0])
  bad = []
  for l in range(nl):
    a, b, wa, wb = int(t['start'][l]), int(t['start'][l + 1]), int(t['wstart'][l]), int(t['wstart'][l + 1])
    c = K.table_layer(t, l)
    got = dict(mask=K.unpack_bits(v['bits'][wa:wb], b - a), bits=v['bits'][wa:wb], counts=counts[l], w=v['w'][a:b], mom=v['mom'][a:b],
               mom2=None, g=v['g'][a:b], noise=None)
    try:
      _check(c, got)
    except AssertionError as e:       # every layer is looked at: the message names all that are wrong
      bad.append((l, t['sizes'][l], str(e)[:200]))
  assert not bad, '%d layers wrong, first: %s' % (len(bad), bad[:3])


def test_layer_table_topk_mask_batched(table):
  """rigl_topk_mask_batched over the table, zero-length entries included: those go through the C ABI directly (an empty
  tensor has no data pointer; the ABI wants one, and never reads it)."""
  from rigl_amd import _lib, ops
  t = table
  nl = len(t['sizes'])
  D = _table_dev(t)
  lib = _lib.load()
  arr = (_lib.TopkLayer * nl)()
  ns = (C.c_int64 * nl)()
  for l in range(nl):
    arr[l].score = D.ptr('score') + 4 * int(t['start'][l])
    arr[l].n = ns[l] = t['sizes'][l]
    arr[l].n_keep = t['n_keep'][l]
    arr[l].mask_bits = D.ptr('bits') + 4 * int(t['wstart'][l])
  ws = ops.workspace(lib.rigl_prune_regrow_workspace_bytes(ns, nl), DEV)
  _lib.check(lib.rigl_topk_mask_batched(arr, nl, C.c_void_p(ws.data_ptr()), ws.numel(), ops._stream()))
  host = D.host()
  assert D.P.guards_intact(host)
  v = D.P.views(host)
  bad = []
  for l in range(nl):
    a, b, wa, wb = int(t['start'][l]), int(t['start'][l + 1]), int(t['wstart'][l]), int(t['wstart'][l + 1])
    if not np.array_equal(v['bits'][wa:wb], K.pack_bits(K.topk_mask_ref(t['score'][a:b], t['n_keep'][l]))):
      bad.append((l, t['sizes'][l], t['n_keep'][l]))
  assert not bad, '%d layers wrong, first (layer, n, k): %s' % (len(bad), bad[:5])
  _same('score (read only)', v['score'], t['score'])


def test_layer_table_magnitude_prune_batched(table):
  """rigl_magnitude_prune_batched over the table's non-empty layers (its ABI refuses n == 0)."""
  from rigl_amd import ops
  t = table
  live = [l for l, n in enumerate(t['sizes']) if n > 0]
  thr0 = (np.arange(len(live)) % 4 * 0.125).astype(F32)
  D = _table_dev(t, dict(thr=thr0, counts=np.zeros(4 * len(live), np.uint32)))
  tw, tb, tt = D.t('w'), D.t('bits'), D.t('thr')
  items = [(tw[int(t['start'][l]):int(t['start'][l + 1])], tb[int(t['wstart'][l]):int(t['wstart'][l + 1])], tt[i:i + 1], t['mag_k'][l])
           for i, l in enumerate(live)]
  ops.magnitude_prune_batched(items, 0.25, counts=D.t('counts'))
  host = D.host()
  assert D.P.guards_intact(host)
  v = D.P.views(host)
  bad = []
  for i, l in enumerate(live):
    a, b, wa, wb = int(t['start'][l]), int(t['start'][l + 1]), int(t['wstart'][l]), int(t['wstart'][l + 1])
    thr, m = PR.mask_update(t['w'][a:b], t['mag_k'][l], thr0[i], 0.25)
    ok = (v['thr'][i:i + 1].view(np.uint32)[0] == np.array([thr], F32).view(np.uint32)[0] and
          np.array_equal(v['bits'][wa:wb], PR.pack_bits(m)) and
          v['counts'][4 * i:4 * i + 4].tolist() == [b - a, t['mag_k'][l], int(m.sum()), int(t['mask'][a:b].sum())])
    if not ok:
      bad.append((l, b - a, t['mag_k'][l]))
  assert not bad, '%d layers wrong, first (layer, n, k): %s' % (len(bad), bad[:5])


def test_repeat_runs_of_the_data_cases_are_identical():
  """The histograms are built with atomics: the result must not depend on their order."""
  cases = [c for c in K.all_k2_cases() if c['frac'] == 0.3][:3] + [K.size_case(8193, True, 1)]
  for c in cases:
    a, b = _run([c], 1)[0], _run([c], 1)[0]
    for key in ('bits', 'w', 'mom', 'counts'):
      np.testing.assert_array_equal(np.asarray(a[key]).view(np.uint32), np.asarray(b[key]).view(np.uint32), err_msg=c['name'])
