"""What the device generation loops that drive emo_grammar_step share (stage1_inference.LeadSheetLoop / LeadSheetQueue, inference.AccompanimentLoop
/ WindowedLoop): the launch's argument block and the draw-score tables behind it, the grammar launch, the running count, the replay phase of a
run and the read-back of the recorded scores.  A subclass brings its tables, its model step (one_step) and what its run() does after the replays."""
import torch

from . import ops
from ._lib import EmoError
from .replay import StepReplayer


def check_vocab(who, V):
    if V > 1024:
        raise EmoError('%s: the device draw takes V <= 1024 (got %d)' % (who, V))


class GrammarLoop:
    """Expects of a subclass: self.dev, self.seq and self.running before _build_block; one_step() before _replay."""
    score_tables = None
    replayed = (0, 0.0)                  # (steps, seconds) of the last run's replays

    def _to_device(self, *arrays):
        """numpy arrays -> their copies on the loop's device."""
        return [torch.from_numpy(a).to(self.dev) for a in arrays]

    def _upload_events(self, flags, beat):
        self.ev_flags, self.ev_beat = self._to_device(flags, beat)

    def _build_block(self, kind, scores, **fields):
        """The grammar launch's argument block (emo_hip.h: emo_grammar_step_t), written once: _gheld keeps what its addresses point to alive,
        the score tables (self.score_tables: ops.draw_score_tables laid out like self.seq, None without `scores`) included.  No tensor of the
        block is allocated again after this: captured graphs hold the raw addresses."""
        self._gargs, self._gheld = ops.GrammarStep(kind=kind), {}
        ops.block_set(self._gargs, self._gheld, **fields)
        self.score_tables = ops.draw_score_tables(self.seq) if scores else None
        if scores:
            ops.block_set(self._gargs, self._gheld, **self.score_tables)

    def grammar(self):
        ops.grammar_step(self._gargs)

    def _live(self):
        """Running count (synchronises)."""
        return int(self.running.item())

    def _replay(self, pos, bound, use_graph, steps_per_graph):
        """one_step() from `pos` until `bound` or until nothing is live, the running count read once per replay (per step without graphs)
        -> the new pos; self.replayed: (steps, seconds) of the replays (the last poll synchronised)."""
        # (the replayer holds graph / graph_k / stream of this run and goes with it: kept on the loop it would close a reference cycle through
        # one_step, and graphs freed by the cycle collector can be freed in the middle of a later capture)
        rp = StepReplayer(self.one_step, self.dev, steps_per_graph)
        pos = rp.run(pos, bound, live=self._live, use_graph=use_graph)
        self.replayed = rp.replayed
        return pos

    def score_arrays(self, tables=None):
        """-> {'logp', 'rank', 'entropy'}: host copies of the loop's score tables (or of `tables`, another loop's).  Needs scores=True."""
        tables = self.score_tables if tables is None else tables
        if tables is None:
            raise EmoError('%s.scores(): the loop was built without scores=True' % type(self).__name__)
        return {k: tables['tok_' + k].cpu().numpy() for k in ('logp', 'rank', 'entropy')}
