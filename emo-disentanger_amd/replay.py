"""The hipGraph replay driver of the device generation loops (generate_streams, and gen_loop.GrammarLoop._replay for LeadSheetLoop,
LeadSheetQueue and AccompanimentLoop): no model or grammar knowledge, only `one_step` — a callable that queues ONE token step whose loop state lives on the device, so that a captured graph continues wherever the
streams are.  A replay costs the device a fixed ~10 us of idle time whatever it holds, so k token steps per replay amortise it (r04:
EMO_GEN_GRAPH_STEPS, default 16); the one-step graph serves the remainder."""
import os
import time

import torch


def graph_steps(k=None):
    """Token steps per replayed graph: the argument, else EMO_GEN_GRAPH_STEPS, else 16; at least 1."""
    return max(1, int(k or os.environ.get('EMO_GEN_GRAPH_STEPS') or 16))


def replay_plan(pos, bound, k):
    """-> (step counts of the replays from `pos` up to `bound` when nothing finishes early, whether a k-step graph is captured at all).
    The k-step graph has to pay for its capture: it exists when at least 2 k steps remain, and is replayed while at least k remain; the
    one-step graph does the rest.  No replay steps past `bound`."""
    left = max(0, bound - pos)
    many = k > 1 and left >= 2 * k
    counts = []
    while left > 0:
        counts.append(k if many and left >= k else 1)
        left -= counts[-1]
    return counts, many


class StepReplayer:
    """run(): one eager step, the replays of replay_plan on a side stream, the eager remainder.  graph / graph_k / stream: the captured one-
    and k-step graphs and the side stream they replay on; replayed: (steps, seconds) of the last run's replay phase."""

    def __init__(self, one_step, device, k=None):
        self.one_step, self.device, self.k = one_step, device, graph_steps(k)
        self.graph = self.graph_k = self.stream = None
        self.replayed = (0, 0.0)

    def capture(self, steps):
        """One graph of `steps` consecutive token steps, captured on the side stream behind everything queued on the current one."""
        if self.stream is None:
            self.stream = torch.cuda.Stream(device=self.device)
        g = torch.cuda.CUDAGraph()
        self.stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.stream):
            with torch.cuda.graph(g, stream=self.stream):
                for _ in range(steps):
                    self.one_step()
        return g

    @torch.no_grad()
    def run(self, pos, bound, live=None, use_graph=True):
        """Steps from `pos` until `bound` or until live() (the count of streams still running; it may synchronise, and raise) is 0 -> the new
        pos.  live is asked once before every replay or eager step; live=None: the step count is fixed and nothing is read back or waited
        for between replays.  The main stream rejoins the side stream also when live raises."""
        def alive():
            return live is None or live() > 0

        self.replayed = (0, 0.0)
        if alive() and pos < bound:
            self.one_step()                      # eager first step (also warms every kernel / workspace cache before any capture)
            pos += 1
        if use_graph and alive() and pos < bound:
            torch.cuda.synchronize()
            counts, many = replay_plan(pos, bound, self.k)
            self.graph = self.capture(1)
            self.graph_k = self.capture(self.k) if many else None
            main = torch.cuda.current_stream()
            t0, p0 = time.perf_counter(), pos
            try:
                with torch.cuda.stream(self.stream):
                    for c in counts:
                        if not alive():
                            break
                        (self.graph_k if c > 1 else self.graph).replay()
                        pos += c
                    else:
                        alive()                  # the poll behind the last replay too: a live that synchronises makes the seconds the device's
            finally:
                main.wait_stream(self.stream)
                self.replayed = (pos - p0, time.perf_counter() - t0)
        while alive() and pos < bound:
            self.one_step()
            pos += 1
        return pos
