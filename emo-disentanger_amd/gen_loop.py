"""What the device generation loops that drive emo_grammar_step share (stage1_inference.LeadSheetLoop / LeadSheetQueue, inference.AccompanimentLoop
/ WindowedLoop): the launch's argument block and the draw-score tables behind it, the grammar launch, the running count, the replay phase of a
run and the read-back of the recorded scores.  A subclass brings its tables, its model step (one_step) and what its run() does after the replays."""
import numbers

import numpy as np
import torch

from . import ops
from ._lib import EmoError
from .replay import StepReplayer


def check_vocab(who, V):
    if V > 1024:
        raise EmoError('%s: the device draw takes V <= 1024 (got %d)' % (who, V))


def mask_words(V):
    """Words of one row of the ban table (emo_hip.h: tok_mask): ceil(V / 32)."""
    return (int(V) + 31) // 32


def pack_token_masks(bans, V):
    """Per-stream bans (None, or ids in [0, V)) -> (tok_mask uint32 [n_masks, mask_words(V)], mask_of int32 [n]) as the grammar launch reads
    them: bit v & 31 of word v >> 5 of row mask_of[r] set = token v is banned for stream r's draws; mask_of[r] = -1: no mask.  Equal bans
    share a row (rows in the order of first use); a stream without a ban, or with an empty one, has none."""
    rows, at, mask_of = [], {}, np.full(len(bans), -1, np.int32)
    for r, ban in enumerate(bans):
        ids = tuple(sorted(set(int(v) for v in ban))) if ban is not None else ()
        if not ids:
            continue
        if ids[0] < 0 or ids[-1] >= V:
            raise ValueError('banned token id %d is outside [0, %d)' % (ids[0] if ids[0] < 0 else ids[-1], V))
        if ids not in at:
            at[ids] = len(rows)
            row = np.zeros(mask_words(V), np.uint32)
            v = np.array(ids, np.int64)
            np.bitwise_or.at(row, v >> 5, (np.uint32(1) << (v & 31).astype(np.uint32)))
            rows.append(row)
        mask_of[r] = at[ids]
    mask = np.stack(rows) if rows else np.zeros((0, mask_words(V)), np.uint32)
    return mask, mask_of


def pack_token_biases(biases, V):
    """Per-stream bias rows (None, or float32 [V]) -> (tok_bias f32 [n_biases, V], bias_of int32 [n]) as the grammar launch reads them
    (emo_hip.h: tok_bias): stream r's draw reads token c's logit as l + tok_bias[bias_of[r], c]; bias_of[r] = -1: no bias.  Equal rows share a
    row of the table (rows in the order of first use), as ban rows do."""
    rows, at, bias_of = [], {}, np.full(len(biases), -1, np.int32)
    for r, b in enumerate(biases):
        if b is None:
            continue
        b = np.ascontiguousarray(b, np.float32)
        if b.shape != (V,):
            raise ValueError('a bias row has shape %s, not (%d,)' % (b.shape, V))
        key = b.tobytes()
        if key not in at:
            at[key] = len(rows)
            rows.append(b)
        bias_of[r] = at[key]
    return (np.stack(rows) if rows else np.zeros((0, V), np.float32)), bias_of


class DrawControls:
    """The per-stream sampling controls of a device generation loop, checked: bans[r] (None, or the sorted ids stream r never draws), temps /
    top_ps (one float per stream, or None where the caller gave one value for all: then `temp` / `top_p`, the launch's scalars, hold), and the
    classifier-free guidance pairs guide_cond / guide_uncond / guide_scale (one entry per stream as emo_hip.h lays them out: (-1, -1, 0.0) for a
    stream without guidance; all three None where no stream is guided).  The soft controls: biases[r] (None, or the float32 [V] row added to
    stream r's logits in the draw; None in place of the list where no stream has one), top_ks / min_ps (one int / float per stream, 0 = off,
    or None where the caller gave none)."""

    def __init__(self, n, V, bans, temp, temps, top_p, top_ps, guide=None, biases=None, top_ks=None, min_ps=None):
        self.n, self.V, self.bans, self.temp, self.temps, self.top_p, self.top_ps = n, V, bans, temp, temps, top_p, top_ps
        self.guide_cond, self.guide_uncond, self.guide_scale = guide if guide is not None else (None, None, None)
        self.biases, self.top_ks, self.min_ps = biases, top_ks, min_ps

    @property
    def soft_arg(self):
        """The soft controls in the form the loop classes take as `soft` (draw_controls' bias / top_k / min_p, per stream), or None."""
        if self.biases is None and self.top_ks is None and self.min_ps is None:
            return None
        return dict(bias=None if self.biases is None else list(self.biases), top_k=None if self.top_ks is None else list(self.top_ks),
                    min_p=None if self.min_ps is None else list(self.min_ps))

    def bias_at(self, r):
        return None if self.biases is None else self.biases[r]

    def top_k_at(self, r):
        return 0 if self.top_ks is None else self.top_ks[r]

    def min_p_at(self, r):
        return 0.0 if self.min_ps is None else self.min_ps[r]

    def soft_key(self, r):
        """What two rows of a guidance pair must share of the soft controls."""
        b = self.bias_at(r)
        return (None if b is None else b.tobytes(), self.top_k_at(r), self.min_p_at(r))

    @property
    def temp_arg(self):
        """What the caller gave as `temp`, in the checked form: the per-stream list, or the one value."""
        return self.temp if self.temps is None else list(self.temps)

    @property
    def top_p_arg(self):
        return self.top_p if self.top_ps is None else list(self.top_ps)

    @property
    def guide_arg(self):
        """The guidance pairs in the form the loop classes take as `guidance`: (cond, uncond, scale) lists, or None."""
        return None if self.guide_cond is None else (list(self.guide_cond), list(self.guide_uncond), list(self.guide_scale))

    def temp_at(self, r):
        return self.temp if self.temps is None else self.temps[r]

    def top_p_at(self, r):
        return self.top_p if self.top_ps is None else self.top_ps[r]

    def guided(self, r):
        """Whether stream r is one row of a guidance pair."""
        return self.guide_cond is not None and self.guide_cond[r] >= 0

    def followers(self):
        """The streams that are the unconditioned row of a pair."""
        return [] if self.guide_cond is None else [r for r in range(self.n) if self.guide_uncond[r] == r]

    def with_guidance(self, scales):
        """scales: one float per stream (0: no guidance) -> the controls of these streams followed by one FOLLOWER per guided stream, in their
        order: a copy of its leader's ban, temp, top_p, bias row, top_k and min_p.  Leader i and its follower g both hold the pair (i, g) and the leader's scale."""
        lead = [i for i in range(self.n) if scales[i] > 0]
        if not lead:
            return self
        assert self.guide_cond is None, 'with_guidance: the streams are guided already'
        out = self.take(list(range(self.n)) + lead)
        cond, unc, sc = [-1] * out.n, [-1] * out.n, [0.0] * out.n
        for j, i in enumerate(lead):
            g = self.n + j
            cond[i], unc[i], sc[i] = cond[g], unc[g], sc[g] = i, g, float(scales[i])
        out.guide_cond, out.guide_uncond, out.guide_scale = cond, unc, sc
        return out

    def take(self, idx):
        """The controls of the streams `idx` (a list of stream indices, repeats allowed), in that order: candidates of an input under best_of,
        the streams a windowed loop takes over.  Guidance pairs are renumbered: the t-th copy of a stream is paired with the t-th copy of its
        partner (ValueError when `idx` splits a pair)."""
        pick = lambda v: None if v is None else [v[i] for i in idx]          # noqa: E731
        guide = None
        if self.guide_cond is not None:
            where, nth = {}, []
            for j, i in enumerate(idx):
                nth.append(len(where.setdefault(i, [])))
                where[i].append(j)

            def at(o, j):
                if o < 0:
                    return -1
                if o not in where or nth[j] >= len(where[o]):
                    raise ValueError('DrawControls.take: stream %d is one row of a guidance pair and its partner %d was not taken with it' % (idx[j], o))
                return where[o][nth[j]]

            guide = ([at(self.guide_cond[i], j) for j, i in enumerate(idx)], [at(self.guide_uncond[i], j) for j, i in enumerate(idx)],
                     [self.guide_scale[i] for i in idx])
            if all(c < 0 for c in guide[0]):
                guide = None
        return DrawControls(len(idx), self.V, [self.bans[i] for i in idx], self.temp, pick(self.temps), self.top_p, pick(self.top_ps), guide,
                            pick(self.biases), pick(self.top_ks), pick(self.min_ps))

    def repeat(self, k):
        """Every stream k times in a row: stream i * k + c has the controls of input i (scoring.best_of_plan's order); copy c of a leader is
        paired with copy c of its follower."""
        return self.take([i for i in range(self.n) for _ in range(k)])

    def tables(self):
        """-> the optional fields of emo_grammar_step_t that are present, as numpy: {'tok_mask' uint32 [n_masks, words], 'mask_of' int32 [n]}
        when a stream has a ban, {'temp_of'} / {'top_p_of'} f32 [n] when the caller gave per-stream values, {'guide_cond', 'guide_uncond' int32
        [n], 'guide_scale' f32 [n]} when a stream is guided, {'tok_bias' f32 [n_biases, V], 'bias_of' int32 [n]} when a stream has a bias (equal
        rows share a row of the table, in the order of first use; -1: none), {'top_k_of'} int32 [n] / {'min_p_of'} f32 [n] when the caller gave
        them.  {} = every new field NULL."""
        out = {}
        if self.biases is not None and any(b is not None for b in self.biases):
            out['tok_bias'], out['bias_of'] = pack_token_biases(self.biases, self.V)
        if self.top_ks is not None:
            out['top_k_of'] = np.array(self.top_ks, np.int32)
        if self.min_ps is not None:
            out['min_p_of'] = np.array(self.min_ps, np.float32)
        if any(b is not None for b in self.bans):
            out['tok_mask'], out['mask_of'] = pack_token_masks(self.bans, self.V)
        if self.temps is not None:
            out['temp_of'] = np.array(self.temps, np.float32)
        if self.top_ps is not None:
            out['top_p_of'] = np.array(self.top_ps, np.float32)
        if self.guide_cond is not None:
            out['guide_cond'], out['guide_uncond'] = np.array(self.guide_cond, np.int32), np.array(self.guide_uncond, np.int32)
            out['guide_scale'] = np.array(self.guide_scale, np.float32)
        return out


def _is_id(v):
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


def _per_input(who, name, value, n, ok, rule):
    """A number for all inputs, or one per input -> (the number, None) or (the first, the list of n floats); each checked by `ok`."""
    if isinstance(value, numbers.Real):
        vals, per = [float(value)], None
    else:
        try:
            vals = [float(v) for v in value]
        except TypeError:
            raise ValueError('%s: %s must be a number or one number per input (got %r)' % (who, name, value))
        if len(vals) != n:
            raise ValueError('%s: %s has %d entries for %d inputs' % (who, name, len(vals), n))
        per = vals
    for v in vals:
        if not ok(v):
            raise ValueError('%s: %s must be %s (got %r)' % (who, name, rule, v))
    return vals[0], per


def _bias_row(who, i, entry, V, event2idx):
    """One bias entry (None, a dict {token id or event name: value}, or a full-length array) -> None or the checked float32 [V] row."""
    if entry is None:
        return None
    if isinstance(entry, dict):
        row = np.zeros(V, np.float32)
        for k, v in entry.items():
            if isinstance(k, str):
                if event2idx is None or k not in event2idx:
                    raise ValueError('%s: bias[%d] names %r, which is no event of the vocabulary' % (who, i, k))
                k = event2idx[k]
            if not _is_id(k) or not 0 <= k < V:
                raise ValueError('%s: bias[%d] has token id %r outside [0, %d)' % (who, i, k, V))
            row[int(k)] = v
    else:
        try:
            row = np.array(entry, np.float32)
        except (TypeError, ValueError):
            raise ValueError('%s: bias[%d] is neither a dict nor an array of %d values' % (who, i, V))
        if row.shape != (V,):
            raise ValueError('%s: bias[%d] has shape %s, a full-length row has (%d,)' % (who, i, row.shape, V))
    if np.isnan(row).any() or (row == np.inf).any():
        raise ValueError('%s: bias[%d] holds NaN or +inf (values are finite, or -inf for a ban)' % (who, i))
    if (row == -np.inf).all():
        raise ValueError('%s: bias[%d] bans every token' % (who, i))
    return row if row.any() else None                          # (all zeros: no bias)


def _bias_rows(who, bias, n, V, event2idx):
    """bias: None, one entry for all inputs (a dict, or a 1-D array of V numbers), or one entry per input -> None or the n checked rows."""
    if bias is None:
        return None
    one = isinstance(bias, dict) or (isinstance(bias, np.ndarray) and bias.ndim == 1 and bias.dtype.kind in 'fiu')
    if not one and not isinstance(bias, np.ndarray):
        bias = list(bias)
        one = len(bias) > 0 and all(isinstance(v, numbers.Real) for v in bias)
    if V is None:
        raise ValueError('%s: a bias needs the vocabulary size' % who)
    if one:
        return [_bias_row(who, 0, bias, V, event2idx)] * n
    if len(bias) != n:
        raise ValueError('%s: bias has %d entries for %d inputs' % (who, len(bias), n))
    rows = [_bias_row(who, i, b, V, event2idx) for i, b in enumerate(bias)]
    return rows if any(r is not None for r in rows) else None


def _per_input_soft(who, name, value, n, conv):
    """top_k / min_p: None, one value for all inputs, or one per input (None in a list: off) -> None or the n checked values."""
    if value is None:
        return None
    if isinstance(value, (numbers.Real, np.generic)):
        return [conv(who, name, value)] * n
    try:
        vals = list(value)
    except TypeError:
        raise ValueError('%s: %s must be a number or one per input (got %r)' % (who, name, value))
    if len(vals) != n:
        raise ValueError('%s: %s has %d entries for %d inputs' % (who, name, len(vals), n))
    return [conv(who, name, 0 if v is None else v) for v in vals]


def _as_top_k(who, name, v):
    if isinstance(v, (bool, np.bool_)) or not (isinstance(v, (numbers.Integral, np.integer)) or (isinstance(v, numbers.Real) and float(v) == int(v))):
        raise ValueError('%s: %s must be an integer (got %r)' % (who, name, v))
    return max(0, min(int(v), 2 ** 31 - 1))


def _as_min_p(who, name, v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (numbers.Real, np.floating)) or float(v) != float(v):
        raise ValueError('%s: %s must be a number, not NaN (got %r)' % (who, name, v))
    return max(0.0, float(v))


def draw_controls(who, n, V, banned=None, temp=1.2, top_p=0.9, guidance=None, bias=None, top_k=None, min_p=None, event2idx=None):
    """The sampling controls of n inputs over a vocabulary of V tokens (read only where there is a ban), checked before anything is allocated
    -> DrawControls.  banned: None (no ban), one sequence of token ids (for every input), or one entry per input, each a sequence of ids or
    None; temp / top_p: a number, or one per input.  ValueError for an id outside [0, V), a ban that leaves no token, a per-input list of the
    wrong length, a temperature <= 0, a top_p outside (0, 1].  guidance: None, or the classifier-free guidance pairs of the n inputs as (guide_cond,
    guide_uncond, guide_scale) lists (emo_hip.h; ops.guide_pairs_error is the rule, ValueError where it is broken, and where the two rows of a
    pair differ in ban, temp, top_p or a soft control).
    The soft controls (emo_hip.h: tok_bias / top_k_of / min_p_of), each None, one value for all inputs, or one per input: bias entries are
    dicts {token id or event name (needs event2idx): value} or full-length arrays of V values, finite or -inf (a ban); top_k an integer (<= 0
    or None: off); min_p a number (<= 0 or None: off).  ValueError for a wrong length, an id outside [0, V), an unknown event name, a NaN or
    +inf bias value, a top_k that is no integer, a min_p that is NaN."""
    biases = _bias_rows(who, bias, n, V, event2idx)
    top_ks = _per_input_soft(who, 'top_k', top_k, n, _as_top_k)
    min_ps = _per_input_soft(who, 'min_p', min_p, n, _as_min_p)
    if banned is None:
        bans = [None] * n
    else:
        banned = list(banned)
        if all(_is_id(v) for v in banned):                       # one ban for every input (an empty one bans nothing)
            bans = [banned] * n
        elif any(_is_id(v) for v in banned):
            raise ValueError('%s: banned mixes token ids and per-input entries' % who)
        elif len(banned) != n:
            raise ValueError('%s: banned has %d entries for %d inputs' % (who, len(banned), n))
        else:
            bans = banned
    checked = []
    for i, ban in enumerate(bans):
        if ban is None:
            checked.append(None)
            continue
        ban = list(ban)
        if not all(_is_id(v) for v in ban):
            raise ValueError('%s: banned[%d] is not a sequence of token ids' % (who, i))
        ids = tuple(sorted(set(int(v) for v in ban)))
        if ids and (ids[0] < 0 or ids[-1] >= V):
            raise ValueError('%s: banned token id %d is outside [0, %d)' % (who, ids[0] if ids[0] < 0 else ids[-1], V))
        if len(ids) >= V:
            raise ValueError('%s: banned[%d] bans every token' % (who, i))
        checked.append(ids or None)
    t, ts = _per_input(who, 'temp', temp, n, lambda v: v > 0 and v == v and v != float('inf'), '> 0')
    p, ps = _per_input(who, 'top_p', top_p, n, lambda v: 0 < v <= 1, 'in (0, 1]')
    ctl = DrawControls(n, V, checked, t, ts, p, ps, None, biases, top_ks, min_ps)
    if guidance is not None:
        cond, unc, scale = ([int(x) for x in guidance[0]], [int(x) for x in guidance[1]], [float(x) for x in guidance[2]])
        bad = ops.guide_pairs_error(cond, unc, scale) if len(cond) == n else 'guide tables of %d rows for %d inputs' % (len(cond), n)
        if bad:
            raise ValueError('%s: %s' % (who, bad))
        for r in range(n):
            o = unc[r] if cond[r] == r else cond[r]
            if cond[r] >= 0 and (ctl.bans[r], ctl.temp_at(r), ctl.top_p_at(r)) != (ctl.bans[o], ctl.temp_at(o), ctl.top_p_at(o)):
                raise ValueError('%s: rows %d and %d of a guidance pair differ in ban, temp or top_p' % (who, r, o))
            if cond[r] >= 0 and ctl.soft_key(r) != ctl.soft_key(o):
                raise ValueError('%s: rows %d and %d of a guidance pair differ in bias, top_k or min_p' % (who, r, o))
        if any(c >= 0 for c in cond):
            ctl.guide_cond, ctl.guide_uncond, ctl.guide_scale = cond, unc, scale
    return ctl


class GrammarLoop:
    """Expects of a subclass: self.dev, self.seq and self.running before _build_block; one_step() before _replay."""
    score_tables = None
    controls = None                      # DrawControls of the loop's streams (None: a loop built without any)
    control_tables = None                # the device tensors behind the block's tok_mask / mask_of / temp_of / top_p_of ({}: all NULL)
    guided_kinds = (ops.GRAMMAR_ACC,)    # the kinds whose block may hold guidance pairs: a lock-step kind that reads them, in a loop that feeds the
                                         # two rows of a pair alike (LeadSheetLoop: GRAMMAR_TXL)
    replayed = (0, 0.0)                  # (steps, seconds) of the last run's replays

    def _to_device(self, *arrays):
        """numpy arrays -> their copies on the loop's device."""
        return [torch.from_numpy(a).to(self.dev) for a in arrays]

    def _upload_events(self, flags, beat):
        self.ev_flags, self.ev_beat = self._to_device(flags, beat)

    def _build_block(self, kind, scores, controls=None, **fields):
        """The grammar launch's argument block (emo_hip.h: emo_grammar_step_t), written once: _gheld keeps what its addresses point to alive,
        the score tables (self.score_tables: ops.draw_score_tables laid out like self.seq, None without `scores`) included, and the tables of
        `controls` (a DrawControls over the streams that `params` holds, or None: self.control_tables, {} where every one of the block's
        optional tok_mask / mask_of / temp_of / top_p_of, tok_bias / bias_of / top_k_of / min_p_of and guide_cond / guide_uncond / guide_scale stays NULL).  No tensor of the block is allocated again after this: captured graphs
        hold the raw addresses."""
        self._gargs, self._gheld = ops.GrammarStep(kind=kind), {}
        ops.block_set(self._gargs, self._gheld, **fields)
        self.controls = controls
        tabs = controls.tables() if controls is not None else {}
        # (any other kind ignores the tables, or its loop does not keep a pair together: the streams would run unguided, silently)
        if 'guide_cond' in tabs and kind not in self.guided_kinds:
            raise EmoError('%s: guidance pairs run in the lock-step launch of a loop that pairs its rows (kind %d is not one of %s)'
                           % (type(self).__name__, kind, list(self.guided_kinds)))
        if 'tok_mask' in tabs:                                   # (torch has no arithmetic on uint32: the words travel as int32, bit for bit)
            tabs['tok_mask'] = tabs['tok_mask'].view(np.int32)
        self.control_tables = dict(zip(tabs, self._to_device(*tabs.values())))
        if tabs:
            ops.block_set(self._gargs, self._gheld, n_masks=len(tabs['tok_mask']) if 'tok_mask' in tabs else 0,
                          n_biases=len(tabs['tok_bias']) if 'tok_bias' in tabs else 0, **self.control_tables)
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
