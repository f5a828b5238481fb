"""Scoring of token sequences under a stage-2 checkpoint: per-token log-probability, rank and predictive entropy (one model forward and one
emo_token_scores launch per batch), per-piece perplexity / top-k accuracy records, and the command line that writes them as scores.json.
Stage-1 lead sheets (the Transformer-XL model) are scored by score_lead_sheet_tokens / score_lead_sheets / --stage 1, below the stage-2 part.

The reference has no scoring tool; what is scored is exactly what its training loss sees — the targets `EventPieceDataset._targets`
builds (stage2_accompaniment/dataloader.py:127-143: only the tokens inside Track_Full spans are predicted, everything else is pad)."""
import contextlib
import json
import math
import os

import numpy as np
import torch

from . import engine, ops

WANT = ('logprob', 'rank', 'entropy')


class TokenScores:
    """score_tokens' result: `logprob`, `rank` (int32), `entropy` as [B, T] device tensors (None when not asked for) and `mask` = dec_target != pad.
    Outside the mask logprob is 0 and rank is -1; entropy is that of the model's prediction at every position."""
    __slots__ = ('logprob', 'rank', 'entropy', 'mask')

    def __init__(self, logprob, rank, entropy, mask):
        self.logprob, self.rank, self.entropy, self.mask = logprob, rank, entropy, mask


def score_tokens(model, dec_input, dec_target, seg_inp=None, want=WANT, pad_token=None):
    """Per-token scores of `dec_target` given `dec_input` (int64 [B, T] on the GPU) under a stage-2 model (MusicPerformer / MusicGPT2): one
    forward in eval mode under no_grad (the model's mode is restored) and one emo_token_scores launch that reads the logits where the
    projection wrote them (its padded buffer included).  pad_token defaults to the model's own ignore index, n_token - 1.

    The forward uses whatever random-feature policy the model is set to: a MusicPerformer that redraws its FAVOR+ projection on every forward
    scores stochastically — two calls differ; build it with redraw='fixed' (or set the redraw probability to 0) for repeatable scores."""
    unknown = set(want) - set(WANT)
    if unknown:
        raise ValueError('score_tokens: unknown output(s) %s (known: %s)' % (sorted(unknown), ', '.join(WANT)))
    pad = model.n_token - 1 if pad_token is None else int(pad_token)
    with eval_mode(model), torch.no_grad():
        logits = model(dec_input, seg_inp=seg_inp)
        V = logits.shape[-1]
        l2 = engine.padded_logits(logits)
        if l2 is None:
            l2 = logits.reshape(-1, V)
        tgt = dec_target.long().reshape(-1)
        engine.check_ids(tgt, V, 'scoring targets', also=pad)
        out = ops.token_scores(l2, tgt, pad, V=V, want=tuple(k for k in ('rank', 'entropy') if k in want))
    shape = dec_target.shape
    return TokenScores(out['nll'].neg().view(shape) if 'logprob' in want else None,
                       out['rank'].view(shape) if 'rank' in want else None,
                       out['entropy'].view(shape) if 'entropy' in want else None,
                       dec_target != pad)


# ------------------------------------------------------------------------------------------------ per-piece records
_FIELDS = ('n_scored', 'nll_sum', 'top1', 'top5', 'entropy_sum')


def piece_record(pid, n_tokens, n_scored, nll_sum, top1, top5, entropy_sum):
    """One scores.json record from a sequence's sums (counts of rank-0 / rank-below-5 targets, sums in nats)."""
    n = int(n_scored)
    mean = nll_sum / n if n else float('nan')
    return {'id': pid, 'n_tokens': int(n_tokens), 'n_scored': n, 'nll_sum': float(nll_sum), 'nll_mean': mean,
            'ppl': math.exp(mean) if n else float('nan'), 'top1': top1 / n if n else float('nan'), 'top5': top5 / n if n else float('nan'),
            'entropy_mean': entropy_sum / n if n else float('nan')}


def corpus_summary(records):
    """Token-weighted totals over the records."""
    n = sum(r['n_scored'] for r in records)
    tot = {k: sum(r[k] * r['n_scored'] for r in records if r['n_scored']) for k in ('top1', 'top5', 'entropy_mean')}
    nll = sum(r['nll_sum'] for r in records)
    s = piece_record('corpus', sum(r['n_tokens'] for r in records), n, nll, tot['top1'], tot['top5'], tot['entropy_mean'])
    s['n_pieces'] = len(records)
    del s['id']
    return s


def _ids_of(batch, B, seen):
    ids = batch.get('piece_id', batch.get('id'))
    if ids is None:
        return list(range(seen, seen + B))
    return [i.item() if torch.is_tensor(i) else i for i in ids]


def score_pieces(model, batches, pad_token, scorer=score_tokens, per_token=None):
    """batches: an iterable of dicts as the data loaders yield them ('dec_input', 'dec_target', 'track_mask'; optional 'piece_id' / 'id' and
    'length').  -> {'pieces': [one record per sequence], 'corpus': token-weighted summary}.  The per-sequence sums are torch reductions over
    [B, T]; one host transfer per batch.  per_token: a callback (id, logprob, rank, entropy) given numpy rows, for the --per-token dump."""
    dev = next(model.parameters()).device
    records = []
    for batch in batches:
        inp, tgt = torch.as_tensor(batch['dec_input']).to(dev), torch.as_tensor(batch['dec_target']).to(dev)
        seg = batch.get('track_mask')
        seg = None if seg is None else torch.as_tensor(seg).to(dev)
        sc = scorer(model, inp, tgt, seg_inp=seg, pad_token=pad_token)
        m = sc.mask
        sums = torch.stack([m.sum(1).double(), -(sc.logprob.double() * m).sum(1), ((sc.rank == 0) & m).sum(1).double(),
                            ((sc.rank >= 0) & (sc.rank < 5) & m).sum(1).double(), (sc.entropy.double() * m).sum(1)], 1).cpu().numpy()
        B = inp.shape[0]
        ids = _ids_of(batch, B, len(records))
        length = batch.get('length')
        n_tok = [int(x) for x in length] if length is not None else (inp != pad_token).sum(1).tolist()
        if per_token is not None:
            lp, rk, en = sc.logprob.cpu().numpy(), sc.rank.cpu().numpy(), sc.entropy.cpu().numpy()
            for b in range(B):
                per_token(ids[b], lp[b], rk[b], en[b])
        for b in range(B):
            records.append(piece_record(ids[b], n_tok[b], *sums[b]))
    return {'pieces': records, 'corpus': corpus_summary(records)}


# ------------------------------------------------------------------------------------------------ targets of a token list
def targets_of(tokens, event2idx, max_len=None, pad_token=None):
    """Input / target / segment arrays (int64) of a generated or dataset token list, by the rule of EventPieceDataset._targets with
    predict_key off and start bar 0: a bar's Track_Full span runs from its Track_Full token to the next Track_LeadSheet token (the last one to
    the end of the list); inside a span the target is the next token and the segment id 1, the last span's final target is EOS; everywhere
    else the target is pad and the segment id 0.  Longer than max_len: built on the whole list, then cut to the first max_len tokens, as the
    dataset does, so fewer targets are scored than the piece has.  pad_token defaults to the id one past the dictionary (load_vocab)."""
    pad = len(event2idx) if pad_token is None else int(pad_token)
    lead, full, eos = event2idx['Track_LeadSheet'], event2idx['Track_Full'], event2idx['EOS_None']
    inp = np.asarray(list(tokens), dtype=np.int64)
    n = len(inp)
    tgt, seg = np.full(n, pad, dtype=np.int64), np.zeros(n, dtype=np.int64)
    starts = np.flatnonzero(inp == full)
    leads = np.flatnonzero(inp == lead)
    for k, a in enumerate(starts):
        last = k == len(starts) - 1
        b = n if last else int(starts[k + 1])
        j = int(np.searchsorted(leads, a))
        if j < len(leads) and leads[j] < b:                      # (a well-formed piece has exactly this boundary in front of every later span)
            b = int(leads[j])
        seg[a:b] = 1
        if not last:
            tgt[a:b] = inp[a + 1:b + 1]
        else:
            tgt[a:b - 1] = inp[a + 1:b]
            tgt[b - 1] = eos
    if max_len is not None:
        inp, tgt, seg = inp[:max_len], tgt[:max_len], seg[:max_len]
    return inp, tgt, seg


def batches_of(token_lists, event2idx, max_len, batch, pad_token=None, ids=None):
    """targets_of for every list, padded to the longest of each group of `batch` (inputs and targets with pad, segments with 0)."""
    pad = len(event2idx) if pad_token is None else int(pad_token)
    for i in range(0, len(token_lists), batch):
        group = token_lists[i:i + batch]
        arrs = [targets_of(t, event2idx, max_len, pad) for t in group]
        T = max(1, max(len(a[0]) for a in arrs))
        inp, tgt, seg = np.full((len(group), T), pad, np.int64), np.full((len(group), T), pad, np.int64), np.zeros((len(group), T), np.int64)
        for r, (a, b, c) in enumerate(arrs):
            inp[r, :len(a)], tgt[r, :len(b)], seg[r, :len(c)] = a, b, c
        yield {'piece_id': list(ids[i:i + batch]) if ids is not None else list(range(i, i + len(group))), 'dec_input': torch.from_numpy(inp),
               'dec_target': torch.from_numpy(tgt), 'track_mask': torch.from_numpy(seg), 'length': [len(t) for t in group]}


def candidate_scores(model, event2idx, candidates, max_len, batch=16, scorer=score_tokens):
    """nll_mean over the Track_Full targets of every candidate token list (an Exception in the list keeps its place and scores NaN)."""
    pad = model.n_token - 1
    real = [i for i, c in enumerate(candidates) if not isinstance(c, Exception)]
    out = [float('nan')] * len(candidates)
    if real:
        recs = score_pieces(model, batches_of([candidates[i] for i in real], event2idx, max_len, batch, pad, ids=real), pad, scorer=scorer)['pieces']
        for r in recs:
            out[r['id']] = r['nll_mean']
    return out


def best_of(scores):
    """Index of the candidate to keep: the lowest nll_mean; a NaN (nothing scored) or an Exception never wins; ties -> the lowest index."""
    best, arg = None, 0
    for i, s in enumerate(scores):
        if isinstance(s, Exception) or s is None or s != s:
            continue
        if best is None or s < best:
            best, arg = s, i
    return arg


_lowest = best_of                       # (for picks_of, whose argument takes the name)


# ------------------------------------------------------------------------------------------------ scores recorded at the draw
BEST_BY = ('forward', 'draws')


def check_best_by(best_by):
    if best_by not in BEST_BY:
        raise ValueError('best_by must be one of %s (got %r)' % (', '.join(repr(b) for b in BEST_BY), best_by))


# ------------------------------------------------------------------------------------------------ the best-of tail of the two generators
def best_of_plan(best_of, best_by, return_scores, *per_input):
    """The checks and the bookkeeping of generate_*(best_of=N, best_by=..., return_scores=...) -> (N, by_draws: the candidates are ranked by
    their recorded draws, want_scores: the loop has to record them, then every list of `per_input` with each entry N times in a row:
    candidate c of input i is entry i * N + c)."""
    n = int(best_of)
    if n < 1:
        raise ValueError('best_of must be at least 1')
    check_best_by(best_by)
    by_draws = n > 1 and best_by == 'draws'
    return (n, by_draws, bool(return_scores or by_draws)) + tuple([x for x in v for _ in range(n)] for v in per_input)


@contextlib.contextmanager
def eval_mode(model):
    """The model in eval mode for the block; the mode it was in comes back at the end, also when the block raises."""
    was_training = model.training
    model.eval()
    try:
        yield
    finally:
        model.train(was_training)


def picks_of(results, nll, best_of, scores=None):
    """The picks of generate_*(best_of=N): candidates i * N .. i * N + N - 1 belong to input i -> per input {'chosen': the index best_of() gives
    for its N nll_mean (the lowest; ties -> the lowest index; a NaN never wins), 'nll_mean', 'candidates'[, 'scores': the N candidates' of
    `scores`]}."""
    picks, n = [], best_of
    for i in range(len(results) // n):
        sl = slice(i * n, (i + 1) * n)
        picks.append({'chosen': _lowest(nll[sl]),'nll_mean': nll[sl], 'candidates': results[sl]})
        if scores is not None:
            picks[-1]['scores'] = scores[sl]
    return picks


def generation_result(results, seconds, scores, picks, return_scores):
    """What generate_lead_sheets / generate_accompaniments return.  picks None (best_of = 1): (results, seconds[, scores]); else (the chosen
    candidates, seconds, picks[, the chosen candidates' scores]); the last element only with return_scores."""
    if picks is None:
        return (results, seconds, scores) if return_scores else (results, seconds)
    chosen = [p['candidates'][p['chosen']] for p in picks], seconds, picks
    return chosen + ([p['scores'][p['chosen']] for p in picks],) if return_scores else chosen


def drawn_mask(logp, rank):
    """Which tokens of a piece were drawn: the cells the grammar launch wrote (the others still hold the sentinels, NaN / -1)."""
    logp, rank = np.asarray(logp, dtype=np.float64), np.asarray(rank)
    return (rank >= 0) & ~np.isnan(logp)


def draw_record(ids, logp, rank, entropy, pid=None):
    """The record of piece_record for one generated piece, from what emo_grammar_step recorded at each draw (generate_*(return_scores=True):
    arrays aligned with `ids`), taken over the DRAWN tokens only: the tokens that were given (primer, injected lead-sheet bars, Track_Full)
    hold sentinels and are skipped.  Sums in float64."""
    logp, entropy, rank = np.asarray(logp, dtype=np.float64), np.asarray(entropy, dtype=np.float64), np.asarray(rank)
    if not (len(logp) == len(rank) == len(entropy) == len(ids)):
        raise ValueError('draw_record: %d ids, %d / %d / %d scores' % (len(ids), len(logp), len(rank), len(entropy)))
    m = drawn_mask(logp, rank)
    return piece_record(pid, len(ids), int(m.sum()), float(-logp[m].sum()), int((rank[m] == 0).sum()), int((rank[m] < 5).sum()),
                        float(entropy[m].sum()))


def draw_scores_mean(scores):
    """Mean -logp over the drawn tokens of every candidate: `scores` as generate_*(return_scores=True) gives them, one {'logp', 'rank',
    'entropy'} per candidate or None for a failed one.  None, and a candidate without a drawn token, score NaN (scoring.best_of never picks
    it over a scored one)."""
    out = []
    for sc in scores:
        if sc is None:
            out.append(float('nan'))
            continue
        m = drawn_mask(sc['logp'], sc['rank'])
        out.append(float(-np.asarray(sc['logp'], dtype=np.float64)[m].mean()) if m.any() else float('nan'))
    return out


def draw_pieces(names, results, scores):
    """One entry per generated piece for write_draw_scores: draw_record plus the per-token arrays (a failed piece: its name and the reason)."""
    out = []
    for name, ids, sc in zip(names, results, scores):
        if sc is None:
            out.append({'id': name, 'failed': 'stuck after 256 rejected samples' if ids is None else str(ids)})
            continue
        rec = draw_record(ids, sc['logp'], sc['rank'], sc['entropy'], pid=name)
        m = drawn_mask(sc['logp'], sc['rank'])
        # (JSON has no NaN: a token that was given holds null in the float rows and -1 in the ranks)
        rec['tokens'] = {'ids': [int(t) for t in ids], 'rank': [int(x) for x in sc['rank']],
                         'logp': [float(x) if k else None for x, k in zip(sc['logp'], m)],
                         'entropy': [float(x) if k else None for x, k in zip(sc['entropy'], m)]}
        out.append(rec)
    return out


def write_draw_scores(path, pieces):
    """The --scores FILE of the two generation command lines: {'pieces': [draw_pieces entries], 'corpus': summary over the scored ones}."""
    scored = [{k: v for k, v in p.items() if k != 'tokens'} for p in pieces if 'failed' not in p]
    for p in pieces:                                                 # (a piece without a drawn token: NaN means -> null, to stay JSON)
        for k, v in list(p.items()):
            if isinstance(v, float) and v != v:
                p[k] = None
    corpus = corpus_summary(scored) if scored else None
    if corpus is not None:
        corpus = {k: (None if isinstance(v, float) and v != v else v) for k, v in corpus.items()}
    with open(path, 'w') as fh:
        json.dump({'pieces': pieces, 'corpus': corpus}, fh, indent=1, allow_nan=False)


# ------------------------------------------------------------------------------------------------ stage 1: lead sheets
def lead_sheet_targets(tokens, lengths, primer_len, pad):
    """Next-token targets of lead sheets: tokens int64 [B, T] (rows padded to T with anything), lengths [B], primer_len an int or [B].
    Position i of row b predicts tokens[b, i + 1] when primer_len - 1 <= i and i + 1 < lengths[b]; every other target is `pad` (the ignore index):
    the positions inside the primer (their next token was given, not generated), the row's last token and everything past it, and a target that
    is `pad` itself.  Works on whatever device `tokens` is on."""
    tokens = torch.as_tensor(tokens).long()
    B, T = tokens.shape
    dev = tokens.device
    lengths = torch.as_tensor(lengths, device=dev).long().reshape(B)
    primer = torch.as_tensor(primer_len, device=dev).long().reshape(-1).expand(B)
    pos = torch.arange(T, device=dev)
    nxt = torch.cat([tokens[:, 1:], tokens.new_full((B, 1), pad)], 1)
    keep = (pos[None, :] >= primer[:, None] - 1) & (pos[None, :] + 1 < lengths[:, None])
    return torch.where(keep, nxt, torch.full_like(nxt, pad))


def score_lead_sheet_tokens(model, tokens, lengths, primer_len, window=None):
    """Per-token scores of lead sheets under a stage-1 model (PlainTransformer): one forward_windowed (eval mode, no_grad; the model's mode is
    restored) and one emo_token_scores launch.  tokens int64 [B, T] on the GPU, rows padded with the model's PAD (n_token - 1, the ignore index);
    targets and mask by lead_sheet_targets.  -> TokenScores [B, T]: entry (b, i) scores token i + 1 of row b.

    What the scores mean: the probabilities a token-by-token pass over the sequence assigns — position i attends to positions
    max(0, i - window) .. i, as generate() / decode_step() do with mem_len = window (default: the model's dec_mem_len) — with no rejected
    draws: the generation loop feeds a rejected draw's predecessor again, which is not part of the piece and not scored.  The generator's first
    call attends fully inside the primer; that is the same band whenever the primer has at most window + 1 tokens (score_lead_sheets reports a
    longer one as primer_outside_window)."""
    pad = model.n_token - 1
    tokens = tokens.long()
    tgt = lead_sheet_targets(tokens, lengths, primer_len, pad)
    with eval_mode(model), torch.no_grad():
        engine.check_ids(tokens, model.n_token, 'lead-sheet tokens')
        logits = model.forward_windowed(tokens.t(), window)               # [T, B, V]: the permuted view of the projection's [B * T, V] rows
        V = logits.shape[-1]
        out = ops.token_scores(logits.permute(1, 0, 2).reshape(-1, V), tgt.reshape(-1), pad, V=V, want=('rank', 'entropy'))
    shape = tgt.shape
    return TokenScores(out['nll'].neg().view(shape), out['rank'].view(shape), out['entropy'].view(shape), tgt != pad)


def lead_sheet_batches(token_lists, primer_lens, batch, pad, ids=None):
    """Groups of `batch` lead sheets, each padded with `pad` to the longest of its group: dicts with 'piece_id', 'tokens' [b, T] int64,
    'length', 'primer_len' (lists)."""
    assert len(primer_lens) == len(token_lists)
    for i in range(0, len(token_lists), batch):
        group = token_lists[i:i + batch]
        T = max(1, max(len(t) for t in group))
        tok = np.full((len(group), T), pad, np.int64)
        for r, t in enumerate(group):
            tok[r, :len(t)] = t
        yield {'piece_id': list(ids[i:i + batch]) if ids is not None else list(range(i, i + len(group))), 'tokens': torch.from_numpy(tok),
               'length': [len(t) for t in group], 'primer_len': [int(p) for p in primer_lens[i:i + batch]]}


def score_lead_sheets(model, token_lists, primer_lens, batch=16, window=None, ids=None, scorer=score_lead_sheet_tokens, per_token=None):
    """One record per lead sheet (the keys of piece_record, and 'primer_outside_window': the primer has more than window + 1 tokens, so the
    generator's first call saw more inside it than the band does — see score_lead_sheet_tokens), in the order given.  token_lists: id lists, primer
    included; primer_lens: how many leading tokens of each were given.  One scorer call and one host transfer per group of `batch`."""
    dev = next(model.parameters()).device
    pad = model.n_token - 1
    window = int(model.dec_mem_len if window is None else window)
    records = []
    for b in lead_sheet_batches(token_lists, primer_lens, batch, pad, ids):
        sc = scorer(model, b['tokens'].to(dev), b['length'], b['primer_len'], window=window)
        m = sc.mask
        sums = torch.stack([m.sum(1).double(), -(sc.logprob.double() * m).sum(1), ((sc.rank == 0) & m).sum(1).double(),
                            ((sc.rank >= 0) & (sc.rank < 5) & m).sum(1).double(), (sc.entropy.double() * m).sum(1)], 1).cpu().numpy()
        if per_token is not None:
            lp, rk, en = sc.logprob.cpu().numpy(), sc.rank.cpu().numpy(), sc.entropy.cpu().numpy()
        for r, pid in enumerate(b['piece_id']):
            if per_token is not None:
                per_token(pid, lp[r], rk[r], en[r])
            rec = piece_record(pid, b['length'][r], *sums[r])
            rec['primer_outside_window'] = b['primer_len'][r] > window + 1
            records.append(rec)
    return records


def lead_sheet_candidate_scores(model, candidates, primer_lens, batch=16, window=None, scorer=score_lead_sheet_tokens):
    """nll_mean over the generated tokens of every candidate lead sheet (None or an Exception in the list keeps its place and scores NaN)."""
    real = [i for i, c in enumerate(candidates) if c is not None and not isinstance(c, Exception)]
    out = [float('nan')] * len(candidates)
    if real:
        for r in score_lead_sheets(model, [candidates[i] for i in real], [primer_lens[i] for i in real], batch, window, ids=real, scorer=scorer):
            out[r['id']] = r['nll_mean']
    return out


def read_lead_sheet_file(path, event2idx):
    """A samp_XX_<emotion>[_roman].txt file as stage1_inference.main writes it: one event per line, WITHOUT the Emotion_<emotion> tag that was
    its one-token primer — the tag comes back from the file name.  (A file that does start with an Emotion_* line is taken as it is.)
    -> (ids, primer_len = 1)."""
    events = [e for e in open(path).read().splitlines() if e]
    if not events or not events[0].startswith('Emotion_'):
        stem = os.path.basename(path).split('.')[0]
        stem = stem[:-len('_roman')] if stem.endswith('_roman') else stem
        tag = 'Emotion_' + stem.split('_')[-1]
        if tag not in event2idx:
            raise ValueError('%s: no Emotion_* line and no emotion in the file name (samp_XX_<emotion>[_roman].txt)' % path)
        events = [tag] + events
    return [event2idx[e] for e in events], 1


# ------------------------------------------------------------------------------------------------ command line
def read_token_file(path, event2idx):
    """A token file as inference.main writes it and read_lead_sheet reads it: one event per line, optionally a Key_* line first (not a token
    of the sequence when the second line is the Emotion_* tag that opens the primer)."""
    events = [e for e in open(path).read().splitlines() if e]
    if len(events) > 1 and 'Key' in events[0] and 'Emotion' in events[1]:
        events = events[1:]
    return [event2idx[e] for e in events]


def _parser():
    import argparse
    ap = argparse.ArgumentParser(description='score token sequences under a stage-2 (or, --stage 1, a stage-1) checkpoint on MI355X')
    ap.add_argument('--stage', type=int, choices=[1, 2], default=2,
                    help='1: lead sheets under the stage-1 Transformer-XL model (-c a stage-1 YAML, --files the samp_*.txt of stage1_inference; no -m, no --split)')
    ap.add_argument('--window', type=int, default=None, help="--stage 1: the attention window (default: the configuration's mem_len)")
    req = ap.add_argument_group('required arguments')
    req.add_argument('-m', '--model_type', choices=['performer', 'gpt2'], help='required with --stage 2')
    req.add_argument('-c', '--configuration', required=True)
    req.add_argument('-r', '--representation', choices=['remi', 'functional'], required=True)
    req.add_argument('--params', required=True, help='checkpoint (.pt state dict)')
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument('--split', choices=['train', 'val'], help="a dataset split of the configuration's data_loader section")
    src.add_argument('--files', nargs='+', help='token files (one event per line)')
    ap.add_argument('--dtype', default=None, choices=[None, 'bf16', 'fp32'])
    ap.add_argument('--batch', type=int, default=8, help='sequences per forward')
    ap.add_argument('-o', '--output', default='scores.json')
    ap.add_argument('--per-token', dest='per_token', default=None, metavar='DIR', help='also write <id>.logprob/.rank/.entropy.npy per piece')
    return ap


def _load_model(args, conf, n_token):
    from . import train as tr
    torch.cuda.set_device(conf['training']['gpuid'])
    model = tr.build_model(args.model_type, n_token, conf['model'], args.dtype).cuda()
    tr.load_pretrained(model, args.params)
    return model.eval()


def _load_stage1_model(args, conf, n_token):
    from .model.plain_transformer import PlainTransformer
    mc, dc = conf['model'], conf['model']['decoder']
    model = PlainTransformer(mc['d_word_embed'], n_token, dc['n_layer'], dc['n_head'], dc['d_model'], dc['d_ff'], dc['tgt_len'], dc['tgt_len'],
                             dec_dropout=dc['dropout'], pre_lnorm=mc['pre_lnorm'], compute_dtype=args.dtype).cuda()
    model.load_state_dict(torch.load(args.params, map_location='cpu'))
    return model.eval()


def _per_token_dump(directory):
    if not directory:
        return None
    os.makedirs(directory, exist_ok=True)

    def dump(pid, lp, rk, en):
        for name, a in (('logprob', lp), ('rank', rk), ('entropy', en)):
            np.save(os.path.join(directory, '%s.%s.npy' % (pid, name)), a)
    return dump


def _main_stage1(args, scorer, load_model):
    """--stage 1: the vocabulary and model of stage1_inference.main (the generator's memory = the configuration's tgt_len, which is the default
    window), the files it writes."""
    import yaml
    from .stage1_inference import read_vocab
    if args.split or not args.files:
        raise SystemExit('--stage 1 scores --files (the samp_*.txt of stage1_inference), not a dataset split')
    conf = yaml.load(open(args.configuration), Loader=yaml.FullLoader)
    event2idx, _, n_token = read_vocab(conf['data']['vocab_path'].format(args.representation))
    window = conf['model']['decoder']['tgt_len'] if args.window is None else args.window
    if window < 1:
        raise SystemExit('--window must be at least 1')
    model = load_model(args, conf, n_token)
    ids = [os.path.splitext(os.path.basename(f))[0] for f in args.files]
    read = [read_lead_sheet_file(f, event2idx) for f in args.files]
    kw = {} if scorer is None else {'scorer': scorer}
    records = score_lead_sheets(model, [r[0] for r in read], [r[1] for r in read], batch=args.batch, window=window, ids=ids,
                                per_token=_per_token_dump(args.per_token), **kw)
    result = {'pieces': records, 'corpus': corpus_summary(records),
              'model': {'type': 'stage1_txl', 'params': args.params, 'dtype': args.dtype, 'window': window}}
    return result


def main(argv=None, scorer=None, load_model=None):
    """-m / -c / -r as inference.main; --params checkpoint; --split {train,val} (through EventPieceDataset, start bar 0) or --files token
    files; writes scores.json ({'pieces': [...], 'corpus': {...}}) and with --per-token DIR three .npy rows per piece.
    --stage 1: -c a stage-1 YAML, -r, --params a stage-1 checkpoint, --files the samp_*.txt files of stage1_inference.main (score_lead_sheets;
    every record also carries primer_outside_window).  scorer / load_model: stand-ins for score_tokens (stage 1: score_lead_sheet_tokens) and
    the model loader."""
    import yaml
    args = _parser().parse_args(argv)
    if args.batch < 1:
        raise SystemExit('--batch must be at least 1')
    if args.stage == 1:
        result = _main_stage1(args, scorer, load_model or _load_stage1_model)
        return _write(args, result)
    if args.model_type is None:
        raise SystemExit('-m/--model_type is required with --stage 2')
    if args.window is not None:
        raise SystemExit('--window goes with --stage 1')
    from .data import EventPieceDataset, load_split, load_vocab
    scorer, load_model = scorer or score_tokens, load_model or _load_model
    conf = yaml.load(open(args.configuration), Loader=yaml.FullLoader)
    dl = conf['data_loader']
    vocab_path = dl['vocab_path'].format(args.representation)
    event2idx, idx2event, pad = load_vocab(vocab_path)
    max_len = conf['model']['max_len']
    model = load_model(args, conf, pad + 1)
    if args.files:
        ids = [os.path.splitext(os.path.basename(f))[0] for f in args.files]
        batches = batches_of([read_token_file(f, event2idx) for f in args.files], event2idx, max_len, args.batch, pad, ids)
    else:
        from torch.utils.data import DataLoader
        ds = EventPieceDataset(data_dir=dl['data_path'].format(args.representation), vocab_file=vocab_path, model_dec_seqlen=max_len,
                               pieces=load_split(dl[args.split + '_split']), pad_to_same=True, appoint_st_bar=0, predict_key=False)
        ds.piece_admissible_stbars = [[0] for _ in ds.pieces]            # score every piece from its first bar (a long one: its first max_len tokens)
        batches = DataLoader(ds, batch_size=args.batch, shuffle=False)
    result = score_pieces(model, batches, pad, scorer=scorer, per_token=_per_token_dump(args.per_token))
    result['model'] = {'type': args.model_type, 'params': args.params, 'dtype': args.dtype,'max_len': max_len}
    return _write(args, result)


def _write(args, result):
    with open(args.output, 'w') as fh:
        json.dump(result, fh, indent=1)
    c = result['corpus']
    print('[score] %d pieces, %d tokens scored: nll %.4f  ppl %.3f  top1 %.4f  top5 %.4f -> %s'
          % (c['n_pieces'], c['n_scored'], c['nll_mean'], c['ppl'], c['top1'], c['top5'], args.output))
    return result


if __name__ == '__main__':
    main()
