"""CPU: the re-anchoring rule of window='rebase' (inference.rebase_plan) on hand-built rows, the stitching of archive and contexts over two
successive phases, and the refusals of generate_accompaniments / parse_args that are raised before anything touches the device."""
import pytest

TLS, TF, X = 7, 8, 3            # Track_LeadSheet, Track_Full, any other event


def _row(primer, bars):
    """primer ids + bars, each Track_LeadSheet, `lead` lead-sheet tokens, Track_Full, `body` drawn tokens -> (row, bar starts)."""
    row, starts = list(primer), []
    for lead, body in bars:
        starts.append(len(row))
        row += [TLS] + [X] * lead + [TF] + [X] * body
    return row, starts


def test_the_cut_lands_on_a_bar_start_and_the_keep_bound_is_exact():
    from emo_disentanger_amd import inference as inf
    row, starts = _row([1, 2, 3], [(2, 6)] * 6)                 # P = 3, bars of 10 tokens at 3, 13, ..., 53; n = 63
    n, P = len(row), 3
    assert starts == [3, 13, 23, 33, 43, 53] and n == 63
    # keep = 33: P + n - b <= 33  <=>  b >= 33: exactly the bar at 33, new_len == keep
    assert inf.rebase_plan(row, n, P, TLS, 33, 96, 2) == (33, 33)
    # one token less room moves the cut to the next bar
    assert inf.rebase_plan(row, n, P, TLS, 32, 96, 2) == (43, 23)
    # one token more in the row (the same keep) moves it too: P + (n + 1) - 33 = 34 > 33
    assert inf.rebase_plan(row + [X], n + 1, P, TLS, 33, 96, 2) == (43, 24)
    for keep in range(13, 64):
        b, new_len = inf.rebase_plan(row, n, P, TLS, keep, 96, 2)
        assert b in starts and new_len == P + n - b <= keep
        assert b == starts[0] or P + n - starts[starts.index(b) - 1] > keep      # the smallest that fits
    assert inf.rebase_plan(row, n, P, TLS, 63, 96, 2) == (3, 63)                  # everything fits: nothing is dropped


def test_fallback_to_the_last_bar_and_the_bar_too_long_error():
    from emo_disentanger_amd import inference as inf
    row, starts = _row([1, 2], [(2, 4), (2, 40)])               # the last bar alone is 44 tokens: P + 44 = 46 > keep
    n, P = len(row), 2
    assert inf.rebase_plan(row, n, P, TLS, 20, 96, 2) == (starts[-1], 46)         # 46 <= 96 - 2 - 2
    assert inf.rebase_plan(row, n, P, TLS, 20, 50, 2) == (starts[-1], 46)         # 46 <= 50 - 2 - 2, exactly
    assert inf.rebase_plan(row, n, P, TLS, 20, 49, 2) == inf.ACC_BAR_TOO_LONG
    assert inf.rebase_plan(row, n, P, TLS, 20, 50, 3) == inf.ACC_BAR_TOO_LONG
    assert inf.rebase_plan([1, 2, X, X], 4, 2, TLS, 20, 96, 2) == inf.ACC_BAR_TOO_LONG   # no bar start at all


def test_a_drawn_track_leadsheet_counts_and_the_primer_is_never_cut():
    from emo_disentanger_amd import inference as inf
    # a primer that itself holds the Track_LeadSheet id: bar starts are looked for from index P on
    row, starts = _row([TLS, TLS, 5], [(1, 3), (1, 3)])
    n, P = len(row), 3
    assert starts == [3, 9]
    assert inf.rebase_plan(row, n, P, TLS, 9, 96, 2) == (9, 9)
    assert inf.rebase_plan(row, n, P, TLS, 15, 96, 2) == (3, 15)
    # the stream's last token is a Track_LeadSheet it has just drawn (its bar not injected yet): a bar start like any other
    row2 = row + [TLS]
    assert inf.rebase_plan(row2, n + 1, P, TLS, 5, 96, 2) == (n, 4)
    b, new_len = inf.rebase_plan(row2, n + 1, P, TLS, 5, 96, 2)
    assert inf.rebase_stitch(row2[:P], [], row2[b:n + 1]) == [TLS, TLS, 5, TLS] and new_len == 4


def test_max_events_goes_down_by_the_tokens_dropped():
    from emo_disentanger_amd import inference as inf
    row, _ = _row([1, 2, 3], [(2, 6)] * 6)
    b, new_len = inf.rebase_plan(row, len(row), 3, TLS, 33, 96, 2)
    me = inf.rebase_max_events(100, b, 3)
    assert me == 100 - 30
    # the reference's limit len(generated) > max_events on the whole piece is the same test on the new context
    for extra in range(0, 60):
        assert (len(row) + extra > 100) == (new_len + extra > me)


def test_archive_and_contexts_of_two_phases_give_back_the_piece():
    from emo_disentanger_amd import inference as inf
    P, keep, W = 3, 33, 64
    piece, _ = _row([1, 2, 3], [(2, 6)] * 14)                   # 143 tokens: what the stream would be without any cut
    ctx, archive, fed, max_events = [], [], 0, 1000
    ctx = piece[:W]
    fed = W
    phases = 0
    while fed < len(piece):
        b, new_len = inf.rebase_plan(ctx, len(ctx), P, TLS, keep, W, 2)
        archive += ctx[P:b]
        max_events = inf.rebase_max_events(max_events, b, P)
        ctx = ctx[:P] + ctx[b:]
        assert len(ctx) == new_len <= keep and ctx[P] == TLS
        take = min(W - len(ctx), len(piece) - fed)              # the phase runs until the window is full again
        ctx += piece[fed:fed + take]
        fed += take
        phases += 1
        assert inf.rebase_stitch(ctx[:P], archive, ctx[P:]) == piece[:fed]
        assert max_events - len(ctx) == 1000 - fed              # the distance to the limit is the whole piece's
    assert phases >= 2


def test_refusals_come_before_any_device_work():
    from emo_disentanger_amd import inference as inf

    class Model:                                                # nothing of it is touched before the refusals
        n_token = 40

    lead, primer = [[[4, 5, 6]] * 3], [[1, 2, 3]]
    with pytest.raises(ValueError, match='window must be'):
        inf.generate_accompaniments(Model(), {}, {}, lead, primer, window='bogus')
    with pytest.raises(ValueError, match='rebase_keep goes with'):
        inf.generate_accompaniments(Model(), {}, {}, lead, primer, window='device', rebase_keep=40)
    W = inf.max_dec_inp_len
    for keep in (4, W - 3 - 2 + 1, 0, -5):                      # below len(primer) + 2 = 5, above W - longest bar - 2
        with pytest.raises(ValueError, match='rebase_keep'):
            inf.generate_accompaniments(Model(), {}, {}, lead, primer, window='rebase', rebase_keep=keep)
    with pytest.raises(ValueError, match='integer'):
        inf.generate_accompaniments(Model(), {}, {}, lead, primer, window='rebase', rebase_keep=40.5)
    assert inf.check_rebase_keep(None, W, 3, 3) == W // 2
    assert inf.check_rebase_keep(5, W, 3, 3) == 5 and inf.check_rebase_keep(W - 5, W, 3, 3) == W - 5
    assert inf.REBASE_TAG != inf.WINDOW_TAG


def test_parse_args_rebase_flags(capsys):
    from emo_disentanger_amd import inference as inf
    base = ['-m', 'gpt2', '-c', 'c.yaml', '-r', 'functional', '-i', 'p.pt', '-o', 'out']
    a = inf.parse_args(base + ['--device', '--window', 'rebase', '--rebase-keep', '512'])
    assert a.window == 'rebase' and a.rebase_keep == 512
    assert inf.parse_args(base + ['--device', '--window', 'rebase']).rebase_keep is None
    for extra, msg in ((['--device', '--rebase-keep', '512'], '--rebase-keep goes with --window rebase'),
                       (['--device', '--window', 'device', '--rebase-keep', '512'], '--rebase-keep goes with --window rebase'),
                       (['--window', 'rebase'], '--window rebase needs --device')):
        with pytest.raises(SystemExit) as e:
            inf.parse_args(base + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err
