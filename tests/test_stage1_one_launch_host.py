"""CPU: the host side of the stage-1 one-launch token step (emo_decode_step, form 2): the head-major hand-off helper, the support predicate
condition by condition, the --step argument and the step= switch."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch


def test_head_major_is_the_numpy_transpose():
    from emo_disentanger_amd.model.plain_transformer import head_major
    n, T, Hh, dh = 3, 7, 8, 64
    x = torch.arange(n * T * Hh * dh, dtype=torch.float32).view(n, T, Hh * dh)
    got = head_major(x, Hh)
    want = x.numpy().reshape(n, T, Hh, dh).transpose(0, 2, 1, 3)
    assert got.shape == (n, Hh, T, dh) and np.array_equal(got.numpy(), want)
    assert got.data_ptr() == x.data_ptr()                            # a view: the hand-off's copy_ does the one transposing copy
    part = head_major(x[:, :5], Hh)                                  # the first T rows of a longer cache, as the hand-off takes them
    assert np.array_equal(part.numpy(), want[:, :, :5])
    dst = torch.zeros(n, Hh, 16, dh)
    dst[:, :, :5].copy_(part)
    assert np.array_equal(dst.numpy()[:, :, :5], want[:, :, :5]) and not dst[:, :, 5:].any()


def _fake(**kw):
    m = dict(_compute_dtype=torch.bfloat16, dec_d_model=512, dec_n_head=8, dec_d_ff=2048, dec_activation='relu', dec_n_layer=12, vocab_size=200,
             dec_mem_len=512, d_word_embed=512, pre_lnorm=True)
    m.update(kw)
    pre = m.pop('pre_lnorm')
    return SimpleNamespace(decoder=SimpleNamespace(pre_lnorm=pre), **m)


def test_support_predicate_names_the_first_failed_condition():
    from emo_disentanger_amd import stage1_inference as s1
    assert s1.one_launch_unsupported(_fake(), 32, device_ok=True) is None
    assert s1.one_launch_unsupported(_fake(dec_n_layer=15, vocab_size=512, dec_mem_len=2047), 1, device_ok=True) is None
    assert s1.one_launch_unsupported(_fake(dec_mem_len=1), 5, device_ok=True) is None
    cases = [(dict(_compute_dtype=torch.float32), 32, 'bf16'), (dict(dec_d_model=256, d_word_embed=256), 32, 'd_model 512'),
             (dict(dec_n_head=4), 32, '8 heads'), (dict(dec_d_ff=1024), 32, 'd_ff 2048'), (dict(pre_lnorm=False), 32, 'pre_lnorm'),
             (dict(dec_activation='gelu'), 32, 'ReLU'), (dict(dec_n_layer=16), 32, '15 layers'), (dict(vocab_size=513), 32, 'vocabulary'),
             (dict(), 33, '1 to 32 streams'), (dict(), 0, '1 to 32 streams'), (dict(dec_mem_len=2048), 32, 'mem_len'),
             (dict(dec_mem_len=4096), 32, 'mem_len'), (dict(dec_mem_len=0), 32, 'mem_len'), (dict(d_word_embed=256), 32, 'd_word_embed')]
    for kw, n, what in cases:
        why = s1.one_launch_unsupported(_fake(**kw), n, device_ok=True)
        assert why is not None and what in why, (kw, n, why)
    assert 'emo_decode_step_supported' in s1.one_launch_unsupported(_fake(), 32, device_ok=False)
    # the FIRST failed condition, in the documented order
    assert 'bf16' in s1.one_launch_unsupported(_fake(_compute_dtype=torch.float32, dec_n_head=4), 40, device_ok=False)
    assert len(s1.one_launch_conditions(_fake(), 32, device_ok=True)) == 12


def test_step_argument_and_switch():
    from emo_disentanger_amd import stage1_inference as s1
    base = ['-c', 'conf.yaml', '-r', 'functional', '-m', 'lead_sheet']
    assert s1.parse_args(base).step == 'chain'
    assert s1.parse_args(base + ['--step', 'one-launch']).step == 'one-launch'
    assert s1.parse_args(base + ['--step', 'chain', '--streams', '8']).streams == 8
    with pytest.raises(SystemExit):
        s1.parse_args(base + ['--step', 'persistent'])
    assert s1.STEPS == ('chain', 'one_launch')
    with pytest.raises(ValueError, match='step must be one of'):
        s1.LeadSheetLoop(None, {}, {}, [['Emotion_Q1']], step='one-launch')       # (the Python spelling has an underscore)
