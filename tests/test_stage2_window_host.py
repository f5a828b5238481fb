"""CPU: the compaction rule of the windowed stage-2 loop on hand-made masks, and the refusal of an unknown `window` before any device work."""
import pytest


def test_compaction_rule_on_hand_made_masks():
    from emo_disentanger_amd.inference import window_compaction as rule
    assert rule([True] * 4) == [0, 1, 2, 3]
    assert rule([True, True, True, False]) == [0, 1, 2, 3]           # 3 of 4 live: more than half, the batch stays
    assert rule([True, False, True, False]) == [0, 2]                # exactly half: the live rows, in order
    assert rule([False, True, True]) == [0, 1, 2]                    # 2 of 3
    assert rule([False, False, True]) == [2]
    assert rule([False, True]) == [1]
    assert rule([True]) == [0]
    assert rule([False] * 3) == []
    live = [False] * 31 + [True]
    assert rule(live) == [31]                                        # one long stream does not carry 31 finished rows
    # a schedule: 8 rows, streams finishing one by one; a kept position is a live one once the batch shrinks, and order is preserved
    rows, done_order, sizes = list(range(8)), [3, 0, 7, 5, 1, 6, 2], []
    finished = set()
    for d in done_order:
        finished.add(d)
        keep = rule([r not in finished for r in rows])
        assert keep == sorted(keep)
        if len(keep) < len(rows):
            assert all(rows[p] not in finished for p in keep) and 2 * len(keep) <= len(rows)
        rows = [rows[p] for p in keep]
        sizes.append(len(rows))
    assert sizes == [8, 8, 8, 4, 4, 2, 1] and rows == [4]


def test_unknown_window_is_refused_before_any_device_work():
    from emo_disentanger_amd import inference as inf
    with pytest.raises(ValueError, match='window'):
        inf.generate_accompaniments(None, {}, {}, [[[1]]], [[0]], window='bogus')
    with pytest.raises(ValueError, match='window'):
        inf.generate_accompaniments(None, {}, {}, [[[1]]], [[0]], window=None)


def test_command_line_refuses_window_device_without_device(capsys):
    from emo_disentanger_amd import inference as inf
    with pytest.raises(SystemExit) as e:
        inf.main(['-m', 'gpt2', '-c', 'none.yaml', '-r', 'functional', '-i', 'none.pt', '-o', 'none', '--window', 'device'])
    assert e.value.code == 2 and '--window device needs --device' in capsys.readouterr().err
