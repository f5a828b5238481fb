"""Stage-1 lead-sheet sampling on PlainTransformer.generate (K/V memory on the HIP relative-position decode kernel).

Behaviour follows /root/reference/stage1_compose/inference_utils.py (generate_plain_xl :51-134, match_emotion_key :137-142) as
pinned by traces of the real loop (tests/golden/txl_generate.json): the first sampled event of the functional / key
representations is the key (temperature 1.1, p 0.97; under key_determine='rule' a non-Key event is an error and a key whose mode
contradicts the emotion is rejected), Beat positions never decrease inside a bar, 256 consecutive rejected samples abort, PAD is
never appended, and a rejected sample makes the loop feed its previous input again — which appends that input to the model's
memory a second time (a reference quirk the traces contain, kept on purpose)."""
import os
import time

import numpy as np
import torch

from . import ops, sampling, scoring
from ._lib import EmoError
from .gen_loop import GrammarLoop, check_vocab, draw_controls
from .inference import _EngineBase, uniform_table
from .sampling import beat_position, event_name, nucleus  # noqa: F401  (`nucleus` is looked up at call time: tests wrap it)

SHARP_NAMES = ('C', 'C#', 'D', 'D#', 'E', 'F', 'F#', 'G', 'G#', 'A', 'A#', 'B')     # pitch-class spelling of convert_key.py:14-15
MAJOR_KEY = np.array(SHARP_NAMES)
MINOR_KEY = np.array([n.lower() for n in SHARP_NAMES])
_MAJOR_MOODS, _MINOR_MOODS = ('Q1', 'Q4', 'Positive'), ('Q2', 'Q3', 'Negative')


def temperature(logits, temperature):
    return sampling.temperature(logits, temperature, longdouble_softmax=True)


def match_emotion_key(emotion, key):
    """High-valence labels go with major keys (upper-case tonic), low-valence ones with minor keys (lower-case tonic)."""
    return (emotion in _MAJOR_MOODS and key in MAJOR_KEY) or (emotion in _MINOR_MOODS and key in MINOR_KEY)


class _LeadSheet:
    """Token list + grammar state of one lead sheet being written."""

    def __init__(self, event2idx, primer, prompt_bars, max_bars, max_events):
        self.tokens = [event2idx['Bar_None']] if primer is None else [event2idx[e] for e in primer]
        self.bars = 0 if (primer is None or prompt_bars is None) else prompt_bars
        self.max_bars, self.max_events = max_bars, max_events
        self.accepted, self.beat, self.rejected_in_a_row = 0, 0, 0
        self.finished, self.stuck = False, False

    def open(self):
        return not self.finished and self.bars < self.max_bars

    def offer(self, word, name):
        """True if `word` (event `name`) was appended."""
        if 'Beat' in name:
            pos = beat_position(name)
            if pos < self.beat:
                self.rejected_in_a_row += 1
                if self.rejected_in_a_row >= 256:
                    self.finished = self.stuck = True
                return False
            self.beat, self.rejected_in_a_row = pos, 0
        if 'Bar' in name:
            self.bars += 1
            self.beat = 0
        if name == 'PAD_None':
            return False
        self.tokens.append(int(word))
        self.accepted += 1
        if len(self.tokens) > self.max_events or name == 'EOS_None':
            self.finished = True
        return True


def generate_plain_xl(model, event2idx, idx2event, max_bars=160, max_events=2048, primer=None, temp=1.2, top_p=0.9, prompt_bars=None,
                      representation='functional', key_determine=None, sampler=None, verbose=False):
    """-> (token ids without the last one, seconds), or (None, seconds) when the model got stuck."""
    note = print if verbose else (lambda *a, **k: None)
    pick = (lambda probs, p: sampler(probs)) if sampler is not None else (lambda probs, p: nucleus(probs, p))
    sheet = _LeadSheet(event2idx, primer, prompt_bars, max_bars, max_events)
    dev = next(model.parameters()).device
    keyed = representation in ('functional', 'key')
    mems = tuple()
    t0 = time.time()
    while sheet.open():
        feed = sheet.tokens if sheet.accepted == 0 else sheet.tokens[-1:]
        logits, mems = model.generate(torch.tensor(feed, dtype=torch.long, device=dev).view(len(feed), 1), mems)
        logits = logits.cpu().numpy()
        if keyed and len(sheet.tokens) == 1:                     # the event after the emotion tag is the key
            word = pick(temperature(logits, 1.1), 0.97)
            name = idx2event[word]
            if key_determine == 'rule':
                kind, _, tonic = name.partition('_')
                if kind != 'Key':
                    raise ValueError('[info] key generation failed')
                if not match_emotion_key(idx2event[sheet.tokens[0]].split('_')[1], tonic):
                    continue
        else:
            word = pick(temperature(logits, temp), top_p)
            name = idx2event[word]
        took = sheet.offer(word, name)
        if sheet.stuck:
            note('[stage1 gen] stuck after 256 rejected samples')
            return None, time.time() - t0
        if took and ('Bar' in name or 'Key' in name):
            note('[stage1 gen] %s: %d bars, %d events' % (name, sheet.bars, len(sheet.tokens)))
    note('[stage1 gen] %d events in %.2f s' % (len(sheet.tokens), time.time() - t0))
    return sheet.tokens[:-1], time.time() - t0


# ------------------------------------------------------------------------------------------------ lock-step batches
# Mirrors of include/emo_hip.h (emo_grammar_step, kind TXL): per-token event bits, per-stream parameter and state words, stream status.
EV_BEAT, EV_BAR, EV_PAD, EV_EOS, EV_KEY, EV_MAJOR, EV_MINOR = 1, 2, 4, 8, 16, 32, 64
P_MAX_BARS, P_MAX_EVENTS, P_PRIMER_LEN, P_KEYED, P_KEY_RULE, P_EMO_MODE = range(6)
S_STATUS, S_LEN, S_ACCEPTED, S_BEAT, S_BARS, S_FAILED, S_FEED, S_DRAWS = range(8)
RUNNING, DONE, STUCK, KEY_ERROR, OVERFLOW, MEM_FULL = range(6)
KEY_TEMP, KEY_TOP_P = 1.1, 0.97                     # the key draw of generate_plain_xl (inference_utils.py:81-82)
_KEY_ERROR = '[info] key generation failed'


def event_tables(idx2event, V):
    """-> (flags int32 [V], beat positions int32 [V]): the reference's own tests of an event name, per token id ('Beat' in e, 'Bar' in e,
    e == 'PAD_None', e == 'EOS_None', e.split('_')[0] == 'Key'; beat_position for Beat events; the key's mode as match_emotion_key sees it).
    Ids without an event get no bits."""
    flags, beat = np.zeros(V, np.int32), np.zeros(V, np.int32)
    for i in range(V):
        e = event_name(idx2event, i)
        if e is None:
            continue
        f = 0
        if 'Beat' in e:
            f |= EV_BEAT
            beat[i] = beat_position(e)
        if 'Bar' in e:
            f |= EV_BAR
        if e == 'PAD_None':
            f |= EV_PAD
        if e == 'EOS_None':
            f |= EV_EOS
        kind, _, tonic = e.partition('_')
        if kind == 'Key':
            f |= EV_KEY
            if match_emotion_key('Positive', tonic):
                f |= EV_MAJOR
            if match_emotion_key('Negative', tonic):
                f |= EV_MINOR
        flags[i] = f
    return flags, beat


def emotion_mode(idx2event, first_token):
    """0 / 1 (major: Q1, Q4, Positive) / 2 (minor: Q2, Q3, Negative) for a stream whose first token is `first_token` (the emotion tag)."""
    parts = idx2event[first_token].split('_')
    emo = parts[1] if len(parts) > 1 else ''
    return 1 if emo in _MAJOR_MOODS else 2 if emo in _MINOR_MOODS else 0


def _per_stream(n, **kw):
    """Keyword values given once or as a list of n: -> n dicts."""
    out = [{} for _ in range(n)]
    for k, v in kw.items():
        vals = list(v) if isinstance(v, (list, tuple)) else [v] * n
        if len(vals) != n:
            raise ValueError('%s: %d values for %d streams' % (k, len(vals), n))
        for d, x in zip(out, vals):
            d[k] = x
    return out


def _draw(sheet, logits, pick, idx2event, keyed, key_rule, temp, top_p):
    """One draw and its grammar, as one iteration of generate_plain_xl (:81-93).  -> True if the word was appended; False if it was
    rejected (a key that contradicts the emotion is rejected before the grammar runs).  Raises ValueError like the reference."""
    if keyed and len(sheet.tokens) == 1:
        word = pick(temperature(logits, KEY_TEMP), KEY_TOP_P)
        name = idx2event[word]
        if key_rule:
            kind, _, tonic = name.partition('_')
            if kind != 'Key':
                raise ValueError(_KEY_ERROR)
            if not match_emotion_key(idx2event[sheet.tokens[0]].split('_')[1], tonic):
                return False
    else:
        word = pick(temperature(logits, temp), top_p)
        name = idx2event[word]
    return sheet.offer(word, name)


def generate_plain_xl_batch(model, event2idx, idx2event, primers, max_bars=160, max_events=2048, temp=1.2, top_p=0.9, prompt_bars=None,
                            representation='functional', key_determine=None, samplers=None, seeds=None):
    """n generate_plain_xl runs in lock-step on ONE TXLMemory, NumPy grammar and sampling per stream.  max_bars, max_events, prompt_bars,
    representation and key_determine may be per-stream lists.  `samplers[i](probs)` defaults to nucleus(probs, p, rng=RandomState(seeds[i]))
    (p = 0.97 on the key draw, top_p otherwise, as generate_plain_xl with its default sampler).  The common primer prefix is one prefill; the
    longer primers' other tokens, and a primer fed again, go one token per step.
    -> (results, seconds): results[i] is what generate_plain_xl(..., sampler=samplers[i]) returns for stream i alone (its id list, or None when
    stuck) or, where that run raises, the exception instance (ValueError of the key rule, EmoError past max_gen_len)."""
    n = len(primers)
    assert n > 0
    kw = _per_stream(n, max_bars=max_bars, max_events=max_events, prompt_bars=prompt_bars, representation=representation, key_determine=key_determine)
    if samplers is None:
        rss = [np.random.RandomState(seeds[i] if seeds is not None else i) for i in range(n)]
        picks = [(lambda probs, p, rs=rs: nucleus(probs, p, rng=rs)) for rs in rss]
    else:
        picks = [(lambda probs, p, f=f: f(probs)) for f in samplers]
    sheets = [_LeadSheet(event2idx, primers[i], kw[i]['prompt_bars'], kw[i]['max_bars'], kw[i]['max_events']) for i in range(n)]
    keyed = [k['representation'] in ('functional', 'key') for k in kw]
    results = [None if s.open() else s.tokens[:-1] for s in sheets]
    live = [s.open() for s in sheets]
    dev = next(model.parameters()).device
    was_training = model.training
    model.eval()
    t0 = time.time()
    try:
        with torch.no_grad():
            from .model.plain_transformer import TXLMemory
            mem = TXLMemory(model, n, model._max_gen_len)
            L0 = min(len(s.tokens) for s in sheets)
            h, _, _ = model._prefill(torch.tensor([s.tokens[:L0] for s in sheets], dtype=torch.long, device=dev).t(), mem)
            logits = model._logits(h.view(n, L0, -1)[:, -1].contiguous())
            pending = [list(s.tokens[L0:]) for s in sheets]
            glen = L0                                                     # positions in the memory (every row advances together)
            while True:
                nxt = [s.tokens[-1] for s in sheets]                      # (rows of finished streams idle)
                logits_np = None
                for i, s in enumerate(sheets):
                    if not live[i]:
                        continue
                    if pending[i]:
                        nxt[i] = pending[i].pop(0)
                        continue
                    if logits_np is None:
                        logits_np = logits.cpu().numpy()
                    try:
                        _draw(s, logits_np[i], picks[i], idx2event, keyed[i], kw[i]['key_determine'] == 'rule', temp, top_p)
                    except ValueError as e:
                        results[i], live[i] = e, False
                        continue
                    if s.stuck or not s.open():
                        results[i], live[i] = (None if s.stuck else s.tokens[:-1]), False
                        continue
                    feed = s.tokens if s.accepted == 0 else s.tokens[-1:]
                    if len(feed) > 1 and model.dec_mem_len > 0 and glen + len(feed) > model.dec_mem_len + 1:
                        results[i], live[i] = NotImplementedError('a multi-token segment that overflows mem_len while it is processed is not built'), False
                        continue
                    nxt[i], pending[i] = feed[0], list(feed[1:])
                if not any(live):
                    break
                if glen >= mem.max_len:
                    for i in range(n):
                        if live[i]:
                            results[i], live[i] = EmoError('generation longer than max_gen_len=%d: construct the model with a larger max_gen_len' % mem.max_len), False
                    break
                logits = model.decode_step(torch.tensor(nxt, dtype=torch.long, device=dev), mem)
                glen += 1
    finally:
        model.train(was_training)
    return results, time.time() - t0


# ------------------------------------------------------------------------------------------------ one-launch token step
STEPS = ('chain', 'one_launch')                     # PlainTransformer.decode_step (a chain of ~88 launches) / emo_decode_step, form 2 (one persistent launch)


def one_launch_conditions(model, n_streams, device_ok=None):
    """What the Transformer-XL form of emo_decode_step was built for, in the order it is reported: [(description, holds)].  device_ok: the answer of
    emo_decode_step_supported() (asked here when None)."""
    dec = model.decoder
    if device_ok is None:
        device_ok = ops.lib.emo_decode_step_supported() == 1
    return [('compute dtype bf16 (got %s)' % str(model._compute_dtype).replace('torch.', ''), model._compute_dtype == torch.bfloat16),
            ('d_model 512 (got %d)' % model.dec_d_model, model.dec_d_model == 512),
            ('8 heads (got %d)' % model.dec_n_head, model.dec_n_head == 8),
            ('d_ff 2048 (got %d)' % model.dec_d_ff, model.dec_d_ff == 2048),
            ('pre_lnorm', bool(dec.pre_lnorm)),
            ('ReLU feed-forward (got %s)' % model.dec_activation, model.dec_activation == 'relu'),
            ('at most 15 layers (got %d)' % model.dec_n_layer, model.dec_n_layer <= 15),
            ('a vocabulary of at most 512 (got %d)' % model.vocab_size, model.vocab_size <= 512),
            ('1 to 32 streams (got %d)' % n_streams, 1 <= n_streams <= 32),
            ('1 <= mem_len and mem_len + 1 <= 2048 (got mem_len %d)' % model.dec_mem_len, 1 <= model.dec_mem_len <= 2047),
            ('d_word_embed == d_model (got %d)' % model.d_word_embed, model.d_word_embed == model.dec_d_model),
            ('a device that holds the launch: 256 compute units with 96 KB of LDS each (emo_decode_step_supported)', bool(device_ok))]


def one_launch_unsupported(model, n_streams, device_ok=None):
    """None, or the first condition of emo_decode_step's Transformer-XL form this model / stream count does not meet."""
    for what, holds in one_launch_conditions(model, n_streams, device_ok):
        if not holds:
            return what
    return None


class OneLaunchStep(_EngineBase):
    """decode_step of n lock-step streams as ONE persistent launch (emo_decode_step, form 2): the packed weights, the pointer table and the workspace
    of the decode engines' one-launch adapter, on a head-major TXLMemory (`mem`).  take_over(prefill memory, T) is the one-time hand-off."""
    step_entry = 'emo_decode_step[txl]'
    _pos_field = 'lens'                                              # the device positions of a step are the streams' lengths

    def __init__(self, model, n_streams, max_len=None, r_dist=None):
        from .model.plain_transformer import TXLMemoryHeadMajor
        why = one_launch_unsupported(model, n_streams)
        if why is not None:
            raise EmoError("step='one_launch' (emo_decode_step[txl]) needs %s; use step='chain'" % why)
        super().__init__(model, n_streams, model._max_gen_len if max_len is None else max_len)
        self.n_pad = (n_streams + 3) // 4 * 4
        self.mem = TXLMemoryHeadMajor(model, n_streams, self.max_len, rows=self.n_pad, r_dist=r_dist)
        self.pos_dev = self.mem.lens                                 # the adapter's device positions ARE the memory's lengths
        self.zeros = torch.zeros(3 * model.dec_d_model, device=self.dev, dtype=torch.float32)      # qkv_net / o_net have no bias
        self._prepare_persist()

    def _inputs(self):
        return self.ps.f32('word_emb.emb_lookup.weight'), None, None      # what PlainTransformer._embed passes: no segment and no positional table

    def _persist_layer(self, l, t_qkv, t_one, t_ffn):
        m, ps, pk = self.model, self.ps, self._pack_fragments
        a, f = 'decoder.layers.%d.dec_attn.' % l, 'decoder.layers.%d.pos_ff.' % l
        nx = 'decoder.layers.%d.dec_attn.' % (l + 1 if l + 1 < m.dec_n_layer else 0)     # (the last layer's slot is loaded and never applied)
        return dict(wqkv=pk(ps.w(a + 'qkv_net.weight'), t_qkv, 4), bqkv=self.zeros,
                    wo=pk(ps.w(a + 'o_net.weight'), t_one, 4), bo=self.zeros,
                    g1=ps.f32(f + 'layer_norm.weight'), be1=ps.f32(f + 'layer_norm.bias'),
                    w1=pk(ps.w(f + 'CoreNet.0.weight'), t_ffn, 4), b1=ps.f32(f + 'CoreNet.0.bias'),
                    w2=pk(ps.w(f + 'CoreNet.3.weight'), t_one, 16), b2=ps.f32(f + 'CoreNet.3.bias'),
                    g2=ps.f32(nx + 'layer_norm.weight'), be2=ps.f32(nx + 'layer_norm.bias'))

    def _persist_state(self, l):
        mem = self.mem
        assert mem.r_dist[l].is_contiguous() and mem.r_dist[l].dtype == torch.bfloat16
        return [mem.r_dist[l].data_ptr(), mem.kc_all[l].data_ptr(), mem.vc_all[l].data_ptr(), 0]      # (the caches live as long as the step object)

    def _check_position(self, pe):
        pass                                                         # (positions are the memory's device lengths; the cache row is clamped in the launch)

    def _persist_form(self):
        m, ps, a0 = self.model, self.ps, 'decoder.layers.0.dec_attn.layer_norm.'
        return dict(form=2, emb_scale=float(m.word_emb.emb_scale), kv_tmax=self.max_len, mem_len=m.dec_mem_len, n_dist=self.mem.r_dist[0].shape[0],
                    ln0=torch.cat([ps.f32(a0 + 'weight'), ps.f32(a0 + 'bias')]).contiguous(),
                    r_w_bias=ps.f32('decoder.r_w_bias').contiguous(), r_r_bias=ps.f32('decoder.r_r_bias').contiguous())

    def take_over(self, mem, T):
        self.mem.take_over(mem, T)
        return self

    @torch.no_grad()
    def step(self, tok, logits_out=None):
        """PlainTransformer.decode_step(tok, self.mem, logits_out): the lengths advance on the device in front of the launch, no host counter takes part
        (capturable); the caller keeps every row below mem.max_len."""
        self.mem.lens.add_(1)
        return self._step_persistent(tok.reshape(-1), None, True, logits_out)


class LeadSheetLoop(GrammarLoop):
    """Device state of generate_lead_sheets: a TXLMemory, the logits of the last step, the uniform table, the grammar tables and
    per-stream parameters / state, the output sequences and the running count; one_step() = emo_grammar_step (kind TXL) + decode_step
    (step='chain') or + emo_decode_step, form 2 (step='one_launch': OneLaunchStep on the head-major copy of the prefill's memory).
    scores=True: the grammar launch (the same one under both steps) also records every accepted draw's log-probability, rank and entropy in
    self.score_tables (ops.draw_score_tables: laid out like seq, sentinels wherever a token was given, not drawn); scores() reads them."""

    def __init__(self, model, event2idx, idx2event, primers, max_bars=160, max_events=2048, temp=1.2, top_p=0.9, prompt_bars=None,
                 representation='functional', key_determine=None, seed=0, step='chain', scores=False, banned=None):
        from .model.plain_transformer import TXLMemory
        self._check_step(model, len(primers), step)
        plens = self._load_jobs(model, event2idx, idx2event, primers, temp, top_p, None, banned, max_bars=max_bars, max_events=max_events,
                                prompt_bars=prompt_bars, representation=representation, key_determine=key_determine)
        n, L0 = self.n, min(plens)
        self.mem = TXLMemory(model, n, model._max_gen_len)
        self.max_len, self.L0 = self.mem.max_len, L0
        self.U = uniform_table(self.max_len - L0 + 1, n, seed, self.dev)      # at most one draw per step, one more at the end
        self.tok = self.seq[:, L0 - 1].contiguous()           # (a valid id in every row before the first grammar step)
        self.logits = torch.empty(n, model.vocab_size, dtype=torch.float32, device=self.dev)
        self._build_block(ops.GRAMMAR_TXL, scores, self.job_controls, **self._block_fields(n))
        with torch.no_grad():
            h, _, _ = model._prefill(self.seq[:, :L0].t(), self.mem)
            self.logits.copy_(model._logits(h.view(n, L0, -1)[:, -1].contiguous()))
        self.stepper = None
        if step == 'one_launch':
            self.stepper = OneLaunchStep(model, n, self.max_len, r_dist=self.mem.r_dist).take_over(self.mem, L0)
            self.mem = self.stepper.mem                              # (the token-major prefill memory goes)
        self.pos = L0                        # positions in the memory (host count: every row advances one per step)

    @staticmethod
    def _check_step(model, rows, step):
        """The refusals of `step` for a model batch of `rows` rows, before anything is allocated; never a silent fall-back to the chain."""
        if step not in STEPS:
            raise ValueError("step must be one of %s (got %r)" % (', '.join(repr(s) for s in STEPS), step))
        if step == 'one_launch':
            why = one_launch_unsupported(model, rows)
            if why is not None:
                raise EmoError("step='one_launch' (emo_decode_step[txl]) needs %s; use step='chain'" % why)

    def _load_jobs(self, model, event2idx, idx2event, primers, temp, top_p, feed, banned=None, **per_stream):
        """n, model, dev and the draw parameters (job_controls: gen_loop.draw_controls of temp / top_p / banned, each one value for all streams
        or one per stream, checked before anything is allocated; temp / top_p: the launch's scalars); the jobs' tables (_job_tables) on the device as seq / params / state, state[FEED] = `feed`
        (None: the shortest primer's length, the prefix a prefill takes); the running count.  -> the primer lengths."""
        n = self.n = len(primers)
        assert n > 0
        kw = _per_stream(n, **per_stream)
        ctl = self.job_controls = draw_controls('generate_lead_sheets', n, model.vocab_size, banned, temp, top_p)
        self.model, self.temp, self.top_p = model, ctl.temp, ctl.top_p
        self.dev = next(model.parameters()).device
        plens, seq, params, state = self._job_tables(model, event2idx, idx2event, primers, kw)
        state[:, S_FEED] = min(plens) if feed is None else feed
        self.seq, self.params, self.state = self._to_device(seq, params, state)
        self.running = torch.tensor([int((state[:, S_STATUS] == RUNNING).sum())], dtype=torch.int32, device=self.dev)
        return plens

    def _block_fields(self, rows):
        """The fields of the grammar launch's block that kinds TXL and TXL_QUEUE share, for a model batch of `rows` rows."""
        return dict(n_rows=rows, n_token=self.model.vocab_size, ld_u=self.n, temperature=self.temp, top_p=self.top_p, key_temperature=KEY_TEMP,
                    key_top_p=KEY_TOP_P, logits=self.logits, u_steps=self.U, ev_flags=self.ev_flags, ev_beat=self.ev_beat, params=self.params,
                    state=self.state, seq=self.seq, tok_out=self.tok, running=self.running)

    def _job_tables(self, model, event2idx, idx2event, primers, kw):
        """The grammar tables of the device (self.ev_flags, self.ev_beat) and, per stream, what the grammar launch reads and keeps
        -> (primer lengths, seq int64 [n, width], params, state int32 [n, 8]: numpy, state[FEED] left to the caller)."""
        n = len(primers)
        sheets = [_LeadSheet(event2idx, primers[i], kw[i]['prompt_bars'], kw[i]['max_bars'], kw[i]['max_events']) for i in range(n)]
        check_vocab('generate_lead_sheets', model.vocab_size)
        self._upload_events(*event_tables(idx2event, model.vocab_size))
        plens = [len(s.tokens) for s in sheets]
        if min(plens) < 1:
            raise ValueError('generate_lead_sheets: empty primer')
        width = max(max(plens), max(k['max_events'] for k in kw)) + 1
        seq = np.zeros((n, width), np.int64)
        params = np.zeros((n, ops.TXL_PARAM_WORDS), np.int32)
        state = np.zeros((n, ops.TXL_STATE_WORDS), np.int32)
        for i, (s, k) in enumerate(zip(sheets, kw)):
            seq[i, :plens[i]] = s.tokens
            params[i, [P_MAX_BARS, P_MAX_EVENTS, P_PRIMER_LEN]] = k['max_bars'], k['max_events'], plens[i]
            params[i, P_KEYED] = k['representation'] in ('functional', 'key')
            params[i, P_KEY_RULE] = k['key_determine'] == 'rule'
            params[i, P_EMO_MODE] = emotion_mode(idx2event, s.tokens[0])
            state[i, [S_STATUS, S_LEN, S_BARS]] = (RUNNING if s.open() else DONE), plens[i], s.bars
        return plens, seq, params, state

    def one_step(self):
        self.grammar()
        if self.stepper is not None:
            self.stepper.step(self.tok, logits_out=self.logits)
        else:
            self.model.decode_step(self.tok, self.mem, logits_out=self.logits)

    def run(self, use_graph=True, steps_per_graph=None):
        """Steps until every stream is finished or the memory is full; the running count is read once per replay (per step without graphs).
        At the memory's end one more grammar step runs alone: a stream that then still wants a model step would overflow max_gen_len."""
        with torch.no_grad():
            self.pos = self._replay(self.pos, self.max_len, use_graph, steps_per_graph)
            if self._live() > 0:
                self.grammar()
            torch.cuda.synchronize()
        if self.stepper is not None:
            self.stepper.check_persistent()                          # a launch that gave up must not pass for a result

    def results(self, idx2event=None):
        """-> per stream: the id list without the last id (DONE), None (STUCK), or the exception the reference loop raises."""
        state, seq = self.state.cpu().numpy(), self.seq.cpu().numpy()
        out = []
        for i in range(self.n):
            st, ln = int(state[i, S_STATUS]), int(state[i, S_LEN])
            if st == DONE:
                out.append([int(t) for t in seq[i, :ln - 1]])
            elif st == STUCK:
                out.append(None)
            elif st == KEY_ERROR:
                out.append(ValueError(_KEY_ERROR))
            else:
                out.append(EmoError('generation longer than max_gen_len=%d: construct the model with a larger max_gen_len' % self.max_len))
        return out

    def scores(self):
        """-> per stream, aligned with results(): {'logp', 'rank', 'entropy'} numpy arrays, one entry per id of the stream's result (NaN / -1 at the
        primer's tokens, which were given), or None where the result is not an id list.  Needs scores=True."""
        tabs, state = self.score_arrays(), self.state.cpu().numpy()
        return [{k: t[i, :int(state[i, S_LEN]) - 1].copy() for k, t in tabs.items()} if int(state[i, S_STATUS]) == DONE else None
                for i in range(self.n)]

    def accepted_tokens(self):
        st = self.state.cpu().numpy()
        return int((st[:, S_LEN] - self.params.cpu().numpy()[:, P_PRIMER_LEN]).sum())


def queue_plan(job_steps, slots):
    """-> (launches, slot occupancy) of a LeadSheetQueue run whose job j holds a slot for job_steps[j] launches (the tokens the model is fed for
    it: its primer, its accepted words, one more per rejected draw).  The first launch only admits: it hands jobs 0 .. slots - 1 out; after that
    the job at the head of the queue goes to the slot that frees up first, in the launch in which its job ends (slots that free up in the same
    launch are interchangeable), so launches = 1 + the time the last slot finishes.  Occupancy = sum(job_steps) / (launches * slots): the
    share of the model's rows that carried a job's token."""
    import heapq
    slots = int(slots)
    if slots < 1:
        raise ValueError('slots must be at least 1')
    steps = [int(x) for x in job_steps]
    if any(x < 0 for x in steps):
        raise ValueError('queue_plan: negative step count')
    free_at = [0] * min(slots, max(len(steps), 1))               # (a slot that never gets a job does not change the end)
    heapq.heapify(free_at)
    end = 0
    for x in steps:
        t = heapq.heappop(free_at) + x
        end = max(end, t)
        heapq.heappush(free_at, t)
    if not steps:
        return 0, 0.0
    launches = 1 + end
    return launches, sum(steps) / float(launches * slots)


class LeadSheetQueue(LeadSheetLoop):
    """LeadSheetLoop for more jobs than rows: `slots` rows of the model batch (one TXLMemory / OneLaunchStep of that many rows) work through
    len(primers) queued jobs.  one_step() = emo_grammar_step (kind TXL_QUEUE) + the model step: a slot whose job ends takes the next job inside
    the grammar launch and restarts its row of the memory (length 0), so the replayed graphs go on and the running count stays the only thing
    read back.  There is no prefill: the first launch admits the first jobs and every primer token goes through the one-token step.  Job j draws
    from column j of the uniform table, whatever slot it lands in.  A job that fills its row of the memory (max_gen_len tokens) ends with
    MEM_FULL, which results() reports like the lock-step loop's bound.  results() / scores() are LeadSheetLoop's, per job; job_steps: the
    launches each finished job held a slot; launches: the launches run() queued (a k-step replay ends up to k - 1 launches past the drain)."""

    def __init__(self, model, event2idx, idx2event, primers, slots, max_bars=160, max_events=2048, temp=1.2, top_p=0.9, prompt_bars=None,
                 representation='functional', key_determine=None, seed=0, step='chain', scores=False, banned=None):
        from .model.plain_transformer import TXLMemory
        slots = self.slots = int(slots)
        if slots < 1:
            raise ValueError('slots must be at least 1 (got %d)' % slots)
        self._check_step(model, slots, step)
        # FEED 1 is what an admission sets: the first token goes out with it
        self._load_jobs(model, event2idx, idx2event, primers, temp, top_p, 1, banned, max_bars=max_bars, max_events=max_events, prompt_bars=prompt_bars,
                        representation=representation, key_determine=key_determine)
        n, dev = self.n, self.dev
        self.stepper = OneLaunchStep(model, slots) if step == 'one_launch' else None
        mem = self.mem = self.stepper.mem if self.stepper is not None else TXLMemory(model, slots, model._max_gen_len)
        self.max_len = mem.max_len
        self.U = uniform_table(mem.max_len, n, seed, dev)            # a job draws at most once per token of its row
        self.tok = self.seq[0, :1].repeat(slots).contiguous()        # (a valid id in every row: a slot that never gets a job feeds it)
        self.logits = torch.zeros(slots, model.vocab_size, dtype=torch.float32, device=dev)
        self.slot_job = torch.full((slots,), -1, dtype=torch.int32, device=dev)
        self.queue_head = torch.zeros(1, dtype=torch.int32, device=dev)
        self.job_steps_dev = torch.zeros(n, dtype=torch.int32, device=dev)
        self._build_block(ops.GRAMMAR_TXL_QUEUE, scores, self.job_controls, n_jobs=n, mem_rows=mem.max_len, slot_job=self.slot_job, queue_head=self.queue_head,
                          mem_lens=mem.lens, job_steps=self.job_steps_dev, **self._block_fields(slots))
        # no job can outlast its row of the memory, so the queue is drained before this many launches whatever the slots do: a budget for the
        # replayer, not a limit that is meant to bind (the per-job limit is the kernel's MEM_FULL)
        self.budget = n * mem.max_len + 2
        self.launches = 0

    def run(self, use_graph=True, steps_per_graph=None):
        """Launches until the running count is 0; it is read once per replay (per step without graphs)."""
        with torch.no_grad():
            self.launches = self._replay(self.launches, self.budget, use_graph, steps_per_graph)
            torch.cuda.synchronize()
            if self._live() > 0:
                raise EmoError('LeadSheetQueue: %d jobs still running after %d launches' % (self._live(), self.launches))
        if self.stepper is not None:
            self.stepper.check_persistent()                          # a launch that gave up must not pass for a result

    def job_steps(self):
        """-> per job, the launches it held a slot (0 for a job that was closed before the run)."""
        return [int(x) for x in self.job_steps_dev.cpu().tolist()]


def generate_lead_sheets(model, event2idx, idx2event, primers, max_bars=160, max_events=2048, temp=1.2, top_p=0.9, prompt_bars=None,
                         representation='functional', key_determine=None, seed=0, use_graph=True, step='chain', best_of=1, best_by='forward',
                         return_scores=False, slots=None, banned=None):
    """The throughput path of generate_plain_xl_batch: the same arguments and result shape, every draw and the grammar on the device
    (emo_grammar_step), each token step = grammar launch + decode_step, k steps captured once as a hipGraph (EMO_GEN_GRAPH_STEPS,
    default 16) and replayed until every stream has finished.  Draws come from a uniform table seeded with `seed` (like generate_streams),
    so the ids are not NumPy-RNG-identical to the reference; they equal the host grammar driven by the same device draws.
    step='one_launch' runs the model step as one persistent launch (emo_decode_step, form 2) and raises EmoError where it was not built for the model.
    -> (results, seconds).

    best_of = N > 1: every primer runs as N streams of the same batch (stream i * N + c is candidate c of primer i; each stream has its own
    column of the uniform table, so the draws differ; per-primer lists among the arguments are repeated alike), every finished candidate is
    scored (scoring.score_lead_sheets: mean negative log-probability of its generated tokens in one windowed forward, window = the model's
    dec_mem_len) and the candidate with the lowest one is returned; ties go to the lowest candidate index, a candidate that failed (stuck, key
    error, out of memory) never wins.  -> (results, seconds, picks), picks[i] = {'chosen': c, 'nll_mean': [N floats, NaN for a failed
    candidate], 'candidates': [N results]}.  best_of = 1 is the path above, draw for draw.

    best_by = 'draws': the candidates are ranked by what the grammar launch recorded at each draw instead (scoring.draw_scores_mean: mean -logp
    over a candidate's drawn tokens, NaN for one that failed or drew nothing); no second forward runs.  The figures are those of the generating
    steps themselves, so they hold for any primer length and are the same under both steps.

    return_scores = True: the result tuple gets one more element at its end, a list aligned with the results: {'logp', 'rank', 'entropy'} numpy
    arrays with one entry per id (NaN / -1 where the id was given: the primer), or None where the result is not an id list.  With best_of > 1
    these are the chosen candidates' and every pick also carries 'scores': the N candidates'.  The ids are those of the call without it.

    slots = None: one lock-step batch with a row per stream (the paths above, draw for draw).  slots = S: the streams (primers times best_of)
    are JOBS that run through S rows (LeadSheetQueue): a row whose job ends takes the next job on the device, so no row idles while jobs wait
    and no batch waits for its longest member; step='one_launch' then has to hold for S rows.  A job draws from its own column of the uniform
    table, so its ids do not depend on S or on the slot it ran in beyond what the model step's arithmetic does; they are not those of slots =
    None, whose streams share a prefill.  The results, best_of, best_by and return_scores are per job as they are per stream.

    banned: None (no ban), one sequence of token ids (no stream ever DRAWS one of them), or one entry per primer, each a sequence of ids or
    None.  The grammar launch reads a banned token's logit as -inf (emo_hip.h: tok_mask), the key draw included, so the ids are those of the
    unbanned call on logits masked that way; primer tokens are fed as they are and the recorded scores stay the model's own (unmasked).
    key_ban() forces a key.  temp / top_p: one value, or one per primer (the key draw keeps its own 1.1 / 0.97).  With best_of = N the N
    candidates of a primer share its ban, temp and top_p; with slots = S they belong to the job.  ValueError, before anything is allocated, for
    an id outside [0, V), a ban that leaves no token, a per-input list of the wrong length, a temp <= 0 or a top_p outside (0, 1]."""
    # a per-primer list among the arguments is repeated like the primers; a value given once holds for every stream
    opts = dict(max_bars=max_bars, max_events=max_events, prompt_bars=prompt_bars, representation=representation, key_determine=key_determine)
    lists = [k for k, v in opts.items() if isinstance(v, (list, tuple)) and len(v) == len(primers)]
    best_of, by_draws, want, primers, *repeated = scoring.best_of_plan(best_of, best_by, return_scores, primers, *(opts[k] for k in lists))
    opts.update(zip(lists, repeated))
    if slots is not None:
        slots = int(slots)
        if slots < 1:
            raise ValueError('slots must be at least 1 (got %d)' % slots)
    # checked per primer, before a loop allocates anything; every candidate of a primer inherits the primer's controls
    ctl = draw_controls('generate_lead_sheets', len(primers) // best_of, model.vocab_size if banned is not None else None, banned, temp,
                        top_p).repeat(best_of)
    t0 = time.time()
    with scoring.eval_mode(model):
        opts.update(temp=ctl.temp_arg, top_p=ctl.top_p_arg, banned=ctl.bans, seed=seed, step=step, scores=want)
        loop = (LeadSheetLoop(model, event2idx, idx2event, primers, **opts) if slots is None else
                LeadSheetQueue(model, event2idx, idx2event, primers, slots, **opts))
        loop.run(use_graph=use_graph)
        out = loop.results()
        sc = loop.scores() if want else None
        picks = None
        if best_of > 1:
            nll = scoring.draw_scores_mean(sc) if by_draws else scoring.lead_sheet_candidate_scores(model, out, loop.params.cpu().numpy()[:, P_PRIMER_LEN].tolist())
            picks = scoring.picks_of(out, nll, best_of, sc if return_scores else None)
    return scoring.generation_result(out, time.time() - t0, sc, picks, return_scores)


def key_ban(event2idx, key):
    """The ids of every Key_* event but `key` (an event of the vocabulary): as `banned` of generate_lead_sheets no other key is ever drawn.
    Under key_determine='rule' a forced key whose mode does not match the emotion is rejected draw after draw, as any such key is."""
    if key not in event2idx or not key.startswith('Key_'):
        raise ValueError('key_ban: %r is not a Key_* event of the vocabulary' % (key,))
    return sorted(i for e, i in event2idx.items() if e.startswith('Key_') and e != key)


def pick_best(model, candidates, primer_lens, best_of, scorer=None):
    """The picks of generate_lead_sheets(best_of=N): candidates i * N .. i * N + N - 1 belong to primer i.  scorer: a stand-in for
    scoring.lead_sheet_candidate_scores (model, candidates, primer_lens) -> nll_mean per candidate."""
    return scoring.picks_of(candidates, (scorer or scoring.lead_sheet_candidate_scores)(model, candidates, primer_lens), best_of)


# ------------------------------------------------------------------------------------------------ command line (reference stage1_compose/inference.py:86-298)
MODES = {'lead_sheet': dict(temp=1.2, top_p=0.97, max_events=512, emotions=('Positive', 'Negative')),
         'full_song': dict(temp=1.1, top_p=0.99, max_events=2400, emotions=('Q1', 'Q2', 'Q3', 'Q4'))}


def read_vocab(vocab_file):
    """stage1_compose/inference.py:22-29: dictionary.pkl = (event2idx, idx2event), PAD appended after it -> (event2idx, idx2event,
    vocab_size).  idx2event[pad] = 'PAD_None' is added as well, so that a sampled PAD is rejected by the grammar instead of raising KeyError."""
    import pickle
    with open(vocab_file, 'rb') as f:
        event2idx, idx2event = pickle.load(f)[:2]
    idx2event = dict(idx2event) if isinstance(idx2event, dict) else dict(enumerate(idx2event))
    pad = len(event2idx)
    event2idx['PAD_None'] = pad
    idx2event[pad] = 'PAD_None'
    return event2idx, idx2event, pad + 1


def parse_args(argv=None):
    """The command line of main()."""
    import argparse
    ap = argparse.ArgumentParser(description='stage-1 lead-sheet generation on MI355X')
    req = ap.add_argument_group('required arguments')
    req.add_argument('-c', '--configuration', required=True, help='a stage-1 YAML (stage1_compose/config keys)')
    req.add_argument('-r', '--representation', choices=['remi', 'functional'], required=True)
    req.add_argument('-m', '--mode', choices=['lead_sheet', 'full_song'], required=True)
    ap.add_argument('-i', '--inference_params', default='best_weight/Functional-two/emopia_lead_sheet_finetune/ep016_loss0.685_params.pt',
                    help='checkpoint (.pt state dict)')
    ap.add_argument('-o', '--output_dir', default='generation/emopia_functional_two')
    ap.add_argument('-n', '--n_groups', type=int, default=20, help='pieces per emotion')
    ap.add_argument('--streams', type=int, default=32, help='pieces generated in lock-step')
    ap.add_argument('--slots', type=int, default=None,
                    help='run ALL jobs (times --best-of) through this many rows of one model batch: a row whose job ends takes the next job on the device '
                         '(device loop only; --streams is not used)')
    ap.add_argument('--dtype', default=None, choices=[None, 'bf16', 'fp32'])
    ap.add_argument('--exact', action='store_true', help='NumPy sampling and grammar on the host (reference-exact per seed) instead of the device loop')
    ap.add_argument('--seed', type=int, default=0, help='seed of the device uniform table (the group of streams j uses seed + j)')
    ap.add_argument('--step', default='chain', choices=['chain', 'one-launch'],
                    help='the model step of the device loop: the chain of launches of decode_step, or one persistent launch (emo_decode_step, form 2)')
    ap.add_argument('--best-of', dest='best_of', type=int, default=1,
                    help='generate N candidates per piece in the same batch (N engine streams each) and keep the likeliest (device loop only)')
    ap.add_argument('--best-by', dest='best_by', default='forward', choices=['forward', 'draws'],
                    help='--best-of: rank the candidates by a scoring forward over the finished pieces, or by the log-probabilities recorded at each draw')
    ap.add_argument('--scores', default=None, metavar='FILE',
                    help='write one JSON record per piece (scoring.draw_record) and its per-token logp / rank / entropy, as recorded at each draw (device loop only)')
    ap.add_argument('--key', default=None, metavar='NAME',
                    help='force the key: a Key_* event of the vocabulary, e.g. Key_C (key_ban: no other key is ever drawn; device loop, functional representation)')
    args = ap.parse_args(argv)
    if args.key is not None and (args.exact or args.representation != 'functional' or not args.key.startswith('Key_')):
        ap.error('--key takes a Key_* event and goes with the device loop (not --exact) and -r functional')
    if args.best_of < 1 or (args.best_of > 1 and args.exact):
        ap.error('--best-of must be at least 1 and goes with the device loop (not --exact)')
    if args.best_by != 'forward' and args.best_of < 2:
        ap.error('--best-by goes with --best-of N, N > 1')
    if args.scores and args.exact:
        ap.error('--scores goes with the device loop (not --exact)')
    if args.slots is not None and (args.slots < 1 or args.exact):
        ap.error('--slots must be at least 1 and goes with the device loop (not --exact)')
    return args


def main(argv=None):
    """Same flags as the reference's stage-1 inference.py (-c -r -m -i -o -n): n_groups pieces for each emotion of the mode, key_determine
    'rule', max_bars 128, written as samp_XX_<emotion>_roman.txt (functional) / samp_XX_<emotion>.txt (remi) without the emotion tag — the
    files the stage-2 command line (inference.main) reads.  All jobs run --streams at a time through generate_lead_sheets (device draws and
    grammar; --step one-launch: the model step as one persistent launch; --slots S: all jobs as one queue through S rows); --exact runs them through generate_plain_xl_batch (NumPy sampling, seeds 0, 1, ... in job order).  MIDI output (miditoolkit,
    relative2absolute) is not part of this package."""
    import yaml
    from .model.plain_transformer import PlainTransformer
    args = parse_args(argv)
    conf = yaml.load(open(args.configuration), Loader=yaml.FullLoader)
    mode = MODES[args.mode]
    max_bars, key_determine = 128, 'rule'
    print('representation: {}, key determine: {}'.format(args.representation, key_determine))
    print('[nucleus parameters] t = {}, p = {}'.format(mode['temp'], mode['top_p']))
    os.makedirs(args.output_dir, exist_ok=True)
    event2idx, idx2event, vocab_size = read_vocab(conf['data']['vocab_path'].format(args.representation))
    mc, dc = conf['model'], conf['model']['decoder']
    model = PlainTransformer(mc['d_word_embed'], vocab_size, dc['n_layer'], dc['n_head'], dc['d_model'], dc['d_ff'], dc['tgt_len'], dc['tgt_len'],
                             dec_dropout=dc['dropout'], pre_lnorm=mc['pre_lnorm'], compute_dtype=args.dtype,
                             max_gen_len=2 * mode['max_events'] + 1024).cuda()
    model.load_state_dict(torch.load(args.inference_params, map_location='cpu'))
    model.eval()
    suffix = '_roman.txt' if args.representation == 'functional' else '.txt'
    jobs = []
    for g in range(args.n_groups):
        for emotion in mode['emotions']:
            out = os.path.join(args.output_dir, 'samp_{:02d}_{}{}'.format(g, emotion, suffix))
            if os.path.exists(out):
                print('[info] {} exists, skipping ...'.format(out))
                continue
            jobs.append((out, emotion))
    print('[# jobs]', len(jobs))
    kw = dict(max_bars=max_bars, max_events=mode['max_events'], temp=mode['temp'], top_p=mode['top_p'], representation=args.representation,
              key_determine=key_determine)
    dev_kw = dict(banned=key_ban(event2idx, args.key)) if args.key is not None else {}
    times, score_pieces = [], []
    want = bool(args.scores)
    per_group = max(1, args.streams // args.best_of)               # --streams counts engine streams: N of them per piece with --best-of N
    if args.slots is not None:
        per_group = max(1, len(jobs))                              # one call: the queue takes every job (seed: that of the first group)
    for j, i in enumerate(range(0, len(jobs), per_group)):
        group = jobs[i:i + per_group]
        primers = [['Emotion_{}'.format(e)] for _, e in group]
        if args.exact:
            res, sec = generate_plain_xl_batch(model, event2idx, idx2event, primers, seeds=list(range(i, i + len(group))), **kw)
        elif args.best_of > 1:
            res, sec, picks, *sc = generate_lead_sheets(model, event2idx, idx2event, primers, seed=args.seed + j, step=args.step.replace('-', '_'),
                                                        best_of=args.best_of, best_by=args.best_by, return_scores=want, slots=args.slots, **kw, **dev_kw)
            for (out, _), p in zip(group, picks):
                print('[info] %s: candidate %d of %d (nll_mean %s)' % (out, p['chosen'], args.best_of, ' '.join('%.4f' % x for x in p['nll_mean'])))
        else:
            res, sec, *sc = generate_lead_sheets(model, event2idx, idx2event, primers, seed=args.seed + j, step=args.step.replace('-', '_'),
                                                 return_scores=want, slots=args.slots, **kw, **dev_kw)
        times.append(sec)
        if want:
            score_pieces += scoring.draw_pieces([os.path.basename(out) for out, _ in group], res, sc[0])
        for (out, _), ids in zip(group, res):
            if ids is None or isinstance(ids, Exception):
                print('[info] %s not written: %s' % (out, 'stuck after 256 rejected samples' if ids is None else ids))
                continue
            with open(out, 'w') as fh:
                fh.write('\n'.join(idx2event[w] for w in ids[1:]) + '\n')
            print('[info] wrote', out, len(ids) - 1, 'events')
    if want:
        scoring.write_draw_scores(args.scores, score_pieces)
        print('[info] wrote', args.scores, len(score_pieces), 'records')
    print('[info] finished {} jobs in {:.2f} s'.format(len(jobs), sum(times)))


if __name__ == '__main__':
    main()
