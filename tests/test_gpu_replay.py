"""GPU: replay.StepReplayer alone, on a toy step (a device counter, optionally a device `running` scalar that drops to 0 when the counter
reaches a given value): the step counts with and without graphs, with a fixed count and with a polled one, and the join of the main stream
behind the side stream when the poll raises.  No model and no project kernel: what can go wrong here is the driver."""
import pytest
import torch

pytestmark = pytest.mark.gpu

K, POS0 = 4, 5
LEFTS = (1, 2, 7, 8, 9, 14)


class _Toy:
    def __init__(self, stop=None, ballast=0):
        dev = self.dev = torch.device('cuda', 0)
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)
        self.running = torch.ones(1, dtype=torch.int32, device=dev)
        self.stop = stop
        self.ballast = torch.ones(ballast, device=dev) if ballast else None      # (makes a step long enough for a missing join to show)
        self.polls = 0

    def one_step(self):
        if self.ballast is not None:
            self.ballast.mul_(1.0)
        self.counter.add_(1)
        if self.stop is not None:
            self.running.sub_((self.counter == self.stop).to(torch.int32))

    def live(self):
        self.polls += 1
        return int(self.running.item())


def _expected_polled(left, stop, use_graph):
    """The rule, stated again: an eager step, then (with graphs) k steps per replay while a k-graph exists (>= 2 k steps were left at capture)
    and >= k remain, else one; a poll before each; without graphs one step per poll."""
    done = 1 if left > 0 else 0
    have_k = use_graph and K > 1 and left - done >= 2 * K
    while done < stop and done < left:
        done += K if have_k and left - done >= K else 1
    return done


@pytest.mark.parametrize('use_graph', [True, False])
@pytest.mark.parametrize('left', LEFTS)
def test_fixed_step_count(left, use_graph):
    from emo_disentanger_amd.replay import StepReplayer
    toy = _Toy()
    rp = StepReplayer(toy.one_step, toy.dev, K)
    pos = rp.run(POS0, POS0 + left, use_graph=use_graph)
    torch.cuda.synchronize()
    assert pos == POS0 + left
    assert int(toy.counter.item()) == left
    assert rp.replayed[0] == (left - 1 if use_graph else 0)
    assert (rp.graph_k is not None) == (use_graph and left - 1 >= 2 * K)


@pytest.mark.parametrize('use_graph', [True, False])
@pytest.mark.parametrize('left', LEFTS)
def test_polled_run_stops_at_the_first_poll_after_zero_and_never_passes_the_bound(left, use_graph):
    from emo_disentanger_amd.replay import StepReplayer
    for stop in (1, 3, 6, 100):
        toy = _Toy(stop=stop)
        rp = StepReplayer(toy.one_step, toy.dev, K)
        pos = rp.run(POS0, POS0 + left, live=toy.live, use_graph=use_graph)
        torch.cuda.synchronize()
        count = int(toy.counter.item())
        assert pos == POS0 + count, (stop, pos, count)
        assert count <= left
        assert count == _expected_polled(left, stop, use_graph), (stop, count)
        if not use_graph:
            assert count == min(stop, left)
        assert toy.polls >= 1


def test_a_poll_that_raises_reaches_the_caller_behind_the_stream_join():
    from emo_disentanger_amd.replay import StepReplayer

    class Stop(Exception):
        pass

    toy = _Toy(ballast=1 << 25)
    rp = StepReplayer(toy.one_step, toy.dev, K)

    def live():
        toy.polls += 1
        if toy.polls == 4:                   # polls: eager step, captures, first replay, second replay
            raise Stop()
        return 1

    with pytest.raises(Stop):
        rp.run(POS0, POS0 + 14, live=live)
    seen = toy.counter.clone()               # queued on the main stream: behind the replay only through the join
    torch.cuda.synchronize()
    assert int(toy.counter.item()) == 1 + K
    assert int(seen.item()) == 1 + K
    assert rp.replayed[0] == K
