"""CPU: the rule by which the generation loops replay their captured token steps (replay.replay_plan: a k-step graph exists when at least 2 k
steps remain and runs while at least k remain, the one-step graph does the rest, nothing steps past the bound), the one reader of
EMO_GEN_GRAPH_STEPS (replay.graph_steps), and generate_streams' refusal of the removed multi-chain mode."""
import pytest

KS = (1, 4, 16)


def _cases():
    for k in KS:
        for left in sorted({0, 1, 2, k - 1, k, 2 * k - 1, 2 * k, 2 * k + 1, 3 * k + 2}):
            yield k, left


@pytest.mark.parametrize('pos', [0, 37])
def test_replay_plan_is_the_rule_of_the_three_loops(pos):
    from emo_disentanger_amd.replay import replay_plan
    for k, left in _cases():
        bound = pos + left
        counts, many = replay_plan(pos, bound, k)
        assert many == (k > 1 and left >= 2 * k), (k, left)
        assert sum(counts) == left, (k, left)
        at = pos
        for c in counts:
            assert c == (k if many and bound - at >= k else 1), (k, left, at)
            at += c
            assert at <= bound, (k, left)
        assert at == bound


def test_replay_plan_past_the_bound_is_empty():
    from emo_disentanger_amd.replay import replay_plan
    assert replay_plan(10, 7, 4) == ([], False)


def test_graph_steps_argument_then_environment_then_16(monkeypatch):
    from emo_disentanger_amd.replay import graph_steps
    monkeypatch.delenv('EMO_GEN_GRAPH_STEPS', raising=False)
    assert graph_steps() == 16 and graph_steps(None) == 16 and graph_steps(4) == 4
    monkeypatch.setenv('EMO_GEN_GRAPH_STEPS', '8')
    assert graph_steps() == 8 and graph_steps(3) == 3
    monkeypatch.setenv('EMO_GEN_GRAPH_STEPS', '0')
    assert graph_steps() == 1
    monkeypatch.setenv('EMO_GEN_GRAPH_STEPS', '-5')
    assert graph_steps() == 1 and graph_steps(-2) == 1


@pytest.mark.parametrize('chains', [2, 0, 4])
def test_generate_streams_refuses_the_removed_chains_mode(chains):
    from emo_disentanger_amd import inference as inf
    with pytest.raises(ValueError, match='multi-chain'):
        inf.generate_streams(None, None, None, 8, chains=chains)       # (refused before the model or a device is touched)
