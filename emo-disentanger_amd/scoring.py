"""Scoring of token sequences under a stage-2 checkpoint: per-token log-probability, rank and predictive entropy (one model forward and one
emo_token_scores launch per batch), per-piece perplexity / top-k accuracy records, and the command line that writes them as scores.json.

The reference has no scoring tool; what is scored is exactly what its training loss sees — the targets `EventPieceDataset._targets`
builds (stage2_accompaniment/dataloader.py:127-143: only the tokens inside Track_Full spans are predicted, everything else is pad)."""
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
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            logits = model(dec_input, seg_inp=seg_inp)
            V = logits.shape[-1]
            l2 = engine.padded_logits(logits)
            if l2 is None:
                l2 = logits.reshape(-1, V)
            tgt = dec_target.long().reshape(-1)
            engine.check_ids(tgt, V, 'scoring targets', also=pad)
            out = ops.token_scores(l2, tgt, pad, V=V, want=tuple(k for k in ('rank', 'entropy') if k in want))
    finally:
        model.train(was_training)
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
    ap = argparse.ArgumentParser(description='score token sequences under a stage-2 checkpoint on MI355X')
    req = ap.add_argument_group('required arguments')
    req.add_argument('-m', '--model_type', choices=['performer', 'gpt2'], required=True)
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


def main(argv=None, scorer=score_tokens, load_model=_load_model):
    """-m / -c / -r as inference.main; --params checkpoint; --split {train,val} (through EventPieceDataset, start bar 0) or --files token
    files; writes scores.json ({'pieces': [...], 'corpus': {...}}) and with --per-token DIR three .npy rows per piece."""
    import yaml
    from .data import EventPieceDataset, load_split, load_vocab
    args = _parser().parse_args(argv)
    if args.batch < 1:
        raise SystemExit('--batch must be at least 1')
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
    dump = None
    if args.per_token:
        os.makedirs(args.per_token, exist_ok=True)

        def dump(pid, lp, rk, en):
            for name, a in (('logprob', lp), ('rank', rk), ('entropy', en)):
                np.save(os.path.join(args.per_token, '%s.%s.npy' % (pid, name)), a)
    result = score_pieces(model, batches, pad, scorer=scorer, per_token=dump)
    result['model'] = {'type': args.model_type, 'params': args.params, 'dtype': args.dtype,'max_len': max_len}
    with open(args.output, 'w') as fh:
        json.dump(result, fh, indent=1)
    c = result['corpus']
    print('[score] %d pieces, %d tokens scored: nll %.4f  ppl %.3f  top1 %.4f  top5 %.4f -> %s'
          % (c['n_pieces'], c['n_scored'], c['nll_mean'], c['ppl'], c['top1'], c['top5'], args.output))
    return result


if __name__ == '__main__':
    main()
