"""GPU tier (-m gpu): a device-resident run stopped after M chunks, saved into one file (surreal_amd/utils/run_state.py)
and continued -- by objects built anew from another seed (run B) and in place by the objects of the uninterrupted run,
their hipGraphs already captured (run C) -- leaves after every later chunk the BYTES the uninterrupted run (run A) leaves:
the learner's whole training state, the replay's tables and counters, the env's state, the polled episodes and the fp64
evaluation returns (run_state_cases.Loop.record).  No tolerance anywhere.

The guard test -- two uninterrupted runs agree -- needs nothing of the feature: it is there so that a resume failure is
not mistaken for a reproducibility failure.

Case 5 (TD3 + LayerNorm on the row schedule): load_train_state_dict writes the parameters with torch copies, which move
torch's write counters, so the packed row weights would be packed again even without invalidate_packed();
test_invalidate_packed_after_a_raw_write shows the hook's own effect with a writer that does not move them."""
import json
import os
import sys

import pytest

import run_state_cases as RC
from run_state_cases import M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

IDS = [c.id for c in RC.CASES]
_RUN_A, _FILES = {}, {}


def run_a(c):
    """run A: 2M chunks uninterrupted -> (its loop, its records); once per case"""
    if c.id not in _RUN_A:
        loop = RC.Loop(c, RC.SEED_A)
        _RUN_A[c.id] = (loop, loop.run(2 * M))
        assert RC.learned(_RUN_A[c.id][1]), [r['learns'] for r in _RUN_A[c.id][1]]
    return _RUN_A[c.id]


def saved_file(c, tmp_path_factory):
    """M chunks of a loop built like run A's, then save_run -> the file; once per case"""
    if c.id not in _FILES:
        path = str(tmp_path_factory.mktemp('run_state') / (c.id + '.pt'))
        loop = RC.Loop(c, RC.SEED_A)
        head = loop.run(M)
        loop.save(path)
        _FILES[c.id] = (path, head)
    return _FILES[c.id]


@pytest.mark.parametrize('cid', IDS)
def test_two_uninterrupted_runs_agree(cid):
    c = RC.BY_ID[cid]
    _, want = run_a(c)
    got = RC.Loop(c, RC.SEED_A).run(2 * M)
    for k in range(2 * M):
        RC.assert_same(got[k], want[k], 'chunk %d' % (k + 1))


@pytest.mark.parametrize('cid', IDS)
def test_resume_into_new_objects(cid, tmp_path_factory):
    """run B: every object built anew after torch.manual_seed of ANOTHER seed, load_run, the load_* calls, M more chunks"""
    c = RC.BY_ID[cid]
    _, want = run_a(c)
    path, head = saved_file(c, tmp_path_factory)
    for k in range(M):
        RC.assert_same(head[k], want[k], 'chunk %d before the save' % (k + 1))
    fresh = RC.Loop(c, RC.SEED_B)
    before = RC.parameters(RC.RS.to_host(fresh.learner.train_state_dict()['tensors']))
    built_a = RC.parameters(RC.RS.to_host(RC.Loop(c, RC.SEED_A).learner.train_state_dict()['tensors']))
    assert before and RC.diff(before, built_a)
    # (the fresh parameters are other ones than a build from run A's seed has)
    fresh.load(path)
    got = fresh.run(M)
    for k in range(M):
        RC.assert_same(got[k], want[M + k], 'chunk %d after the resume' % (M + k + 1))


@pytest.mark.parametrize('cid', IDS)
def test_resume_in_place(cid, tmp_path_factory):
    """run C: run A's own objects after chunk 2M load the file and run M chunks again"""
    c = RC.BY_ID[cid]
    loop, want = run_a(c)
    path, _ = saved_file(c, tmp_path_factory)
    if c.algo == 'ddpg':
        assert loop.learner._ws is not None and (not loop.learner.use_graph or loop.learner._ws.graph is not None)
        step_word, packed = loop.learner._ws.step, getattr(loop.learner._ws, 'rows_packed', None)
        if c.opts.get('rows'):
            assert loop.learner._schedule(loop.B, c.D) == 'rows' and packed is not None
    tables = {k: t.data.data_ptr() for k, t in loop.replay._tables.items()}
    loop.load(path)
    assert {k: t.data.data_ptr() for k, t in loop.replay._tables.items()} == tables      # (in place)
    if c.algo == 'ddpg':
        ws = loop.learner._ws
        assert ws.step is step_word and int(ws.step.item()) == loop.learner.critic_step == ws.dev_step
        assert getattr(ws, 'rows_versions', None) is None
    got = loop.run(M)
    for k in range(M):
        RC.assert_same(got[k], want[M + k], 'chunk %d after the in-place restore' % (M + k + 1))


@pytest.mark.parametrize('cid', IDS)
def test_a_save_is_pure(cid, tmp_path):
    c = RC.BY_ID[cid]
    _, want = run_a(c)
    got = RC.Loop(c, RC.SEED_A).run(2 * M, save_each=str(tmp_path / 'every_chunk.pt'))
    for k in range(2 * M):
        RC.assert_same(got[k], want[k], 'chunk %d' % (k + 1))


def test_invalidate_packed_after_a_raw_write():
    """the row schedule's packed weights after a write that does not move torch's write counters (through .data: what a
    raw-pointer writer looks like to torch): with invalidate_packed() the next iterations are those of a learner that
    loaded the same state; without it they are not"""
    c = RC.BY_ID['ddpg-td3-ln-rows-drift']

    def third_chunk(how):
        """two chunks, then both critics' and the actor's parameters halved by writer `how`, then a third chunk"""
        lp = RC.Loop(c, RC.SEED_A)
        lp.run(2)
        L = lp.learner
        assert L._schedule(lp.B, c.D) == 'rows' and L._ws.rows_versions == L._rows_versions()
        live = L._train_tensors()
        for k in ('model.ac_flat', 'model2.critic_flat'):
            new = live[k] * 0.5
            if how == 'torch':
                live[k].copy_(new)                              # (moves torch's write counter: packed again by itself)
            else:
                versions = L._rows_versions()
                live[k].data.copy_(new)
                assert L._rows_versions() == versions
        if how == 'raw, invalidated':
            L.invalidate_packed()
        return lp.run(1)[0]['learner']['tensors']
    want = third_chunk('torch')
    assert not RC.diff(third_chunk('raw, invalidated'), want)
    assert RC.diff(third_chunk('raw'), want)


@pytest.mark.parametrize('algo', ['ppo', 'ddpg'])
def test_env_state_alone(algo):
    """save after 3 + 4 steps; a fresh env loaded from the save and stepped 5 more leaves in a fresh-but-loaded replay the
    bytes one env stepped 3 + 4 + 5 leaves"""
    c = RC.BY_ID['ppo-lstm-adapt-reach' if algo == 'ppo' else 'ddpg-ou-reach']

    def build():
        lp = RC.Loop(c, RC.SEED_A)
        roll = lp.venv.ppo_rollout_into if algo == 'ppo' else lp.venv.ddpg_rollout_into
        return lp, (lambda steps: roll(lp.agent, lp.replay, steps))
    one, step = build()
    for k in (3, 4, 5):
        step(k)
    two, step = build()
    for k in (3, 4):
        step(k)
    saved = RC.RS.to_host(dict(env=two.venv.state_dict(), replay=two.replay.state_dict(), agent=two.agent.state_dict()))
    three, step = build()
    three.replay.load_state_dict(saved['replay'])
    three.venv.load_state_dict(saved['env'])
    three.agent.load_state_dict(saved['agent'])
    step(5)
    for lp in (one, three):
        lp.monitor.poll()
    RC.assert_same(RC.RS.to_host(three.replay.state_dict()), RC.RS.to_host(one.replay.state_dict()), 'replay')
    RC.assert_same(RC.RS.to_host(three.venv.state_dict()), RC.RS.to_host(one.venv.state_dict()), 'env')
    RC.assert_same(RC.RS.to_host(three.agent.state_dict()), RC.RS.to_host(one.agent.state_dict()), 'agent')


WALL_CLOCK = ('wall_s', 'eval_device_s', 'eval_per_step_s')


def _lines(lines):
    """the logged lines without their wall-clock fields (seconds measured by the run itself: no two runs share them), as
    strings again"""
    out = []
    for s in lines:
        d = json.loads(s)
        out.append(json.dumps({k: v for k, v in d.items() if k not in WALL_CLOCK}))
    return out


@pytest.mark.parametrize('algo', ['ppo', 'ddpg'])
def test_train_reach_resumes(algo, tmp_path):
    """scripts/train_reach.py: 6 chunks uninterrupted against 3 chunks with --save, then --resume: from chunk 4 on the
    logged lines are the same strings (wall-clock fields apart)"""
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import train_reach as TR
    kw = dict(iters=6, eval_every=2, device_eval=True, random_resets=True, seed=0)
    whole, head, tail = [], [], []
    TR.train(algo, log=whole.append, **kw)
    path = str(tmp_path / 'run.pt')
    TR.train(algo, log=head.append, save=path, **dict(kw, iters=3))
    TR.train(algo, log=tail.append, resume=path, **kw)
    # the uninterrupted run: the baselines, then the evaluations at 0, 2, 4, 6; the resumed one: those at 4 and 6
    assert len(whole) == 5 and len(tail) == 2
    assert [json.loads(s)['iteration'] for s in tail] == [4, 6]
    assert json.loads(tail[-1])['learner_iterations'] > json.loads(whole[2])['learner_iterations'] > 0
    assert _lines(tail) == _lines(whole[3:])
    assert _lines(head[1:3]) == _lines(whole[1:3])                  # (the baseline line carries --iters)
