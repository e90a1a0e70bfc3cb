"""The unfused fp32 Conformer block (walk_block_rows in csrc/model.h) and its three callers, pinned by launch counts per
MI355ASR_K_* category (mi355asr_profile_read): run_block_rows under MI355ASR_FUSED=0, the single-stream ChunkConformer calls
and the batched streams.  The counts follow from the code: a rows block with self-attention is FFModule 1, qkv, attention,
out-projection, GLU, depthwise conv, conv tail, FFModule 2 -- one launch each -- and none of the fused categories; the stacks
add one projection and one head where they have them, the streaming fronts one launch per front stage.

The switch of case (a) is read once per process, so that case runs in a child: `python tests/test_gpu_rows_walker.py rows_block`."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

# the MI355ASR_K_* categories of include/mi355asr.h
K = dict(STFT=0, UTT_MAX=1, MEL=2, SUBCONV=3, SUBLINEAR=4, FFN=5, QKV=6, ATTN=7, ATTN_OUT=8, PW1_GLU=9, DWCONV=10, CONV_TAIL=11,
         CTC_PROJECT=12, CTC_HEAD=13, COLLAPSE=14, FF1_QKV=15, OUT_GLU=16, TAIL_FF2=17, TAIL_FF1=18, ENC_STACK=19)
ROWS_BLOCK = dict(FFN=2, QKV=1, ATTN=1, ATTN_OUT=1, PW1_GLU=1, DWCONV=1, CONV_TAIL=1, FF1_QKV=0, OUT_GLU=0, TAIL_FF1=0, TAIL_FF2=0)
FRONT = dict(STFT=1, MEL=1, SUBCONV=1, SUBLINEAR=1)


def assert_counts(what, counts, blocks, **others):
    """`blocks` rows blocks, the categories of `others`, and nothing else"""
    want = dict({k: 0 for k in K}, **{k: v * blocks for k, v in ROWS_BLOCK.items()})
    want.update(others)
    got = {k: counts[i] for k, i in K.items()}
    print("%s: %s" % (what, {k: v for k, v in got.items() if v}))
    assert got == want, (what, {k: (got[k], want[k]) for k in K if got[k] != want[k]})


def arrays(r):
    """every tensor / array / number of a result, in order"""
    import torch
    if isinstance(r, dict):
        return [a for k in sorted(r) for a in arrays(r[k])]
    if isinstance(r, (tuple, list)):
        return [a for v in r for a in arrays(v)]
    if r is None:
        return []
    return [r.cpu().numpy() if torch.is_tensor(r) else np.asarray(r)]


def assert_same_bits(what, r0, r1):
    a, b = arrays(r0), arrays(r1)
    assert len(a) == len(b) and len(a) > 0, what
    for i, (u, v) in enumerate(zip(a, b)):
        assert u.shape == v.shape and np.array_equal(u, v), "%s: output %d differs between two runs from the same state" % (what, i)


@functools.lru_cache(maxsize=None)
def chunk_case():
    """the SMALL ChunkConformer of test_gpu_chunk_streams.py with a blank bias that picks every frame, and two audios"""
    import oracle.conformer_oracle as co
    from test_gpu_chunk_streams import SMALL, gated_waves, model
    w = co.chunk_weights(SMALL, seed=3)
    w["picker/fully_connected/bias"][-1] = -20.0
    return model(SMALL, w), gated_waves(2, 3), SMALL


def picker_packet(m, x):
    from test_gpu_chunk_streams import W
    return m.picker_stream_predict(x[0][None, :W, None], m.init_picker_caches(1))


# ---- (a) run_block_rows -------------------------------------------------------------------------------------------------------
def step_rows_block():
    """conformer_block(0, x) of the small encoder, B = 2, T = 32: 64 rows, above the 48 of MI355ASR_SMALL_M, so MI355ASR_FUSED=0
    sends the block to run_block_rows"""
    assert os.environ.get("MI355ASR_FUSED") == "0" and "MI355ASR_SMALL_M" not in os.environ
    from caller_contract_gpu_steps import profile_counts
    from helpers import co, encoder_kwargs, small_cfg
    from tensorflowasr_amd.models import ConformerEncoder
    cfg = small_cfg(2)
    e = ConformerEncoder(**encoder_kwargs(cfg))
    e.load_weights(co.encoder_weights(cfg, seed=3), by_name=False)
    x = np.random.default_rng(5).standard_normal((2, 32, 144)).astype(np.float32)
    assert_counts("rows block", profile_counts(e._h, lambda: e.conformer_block(0, x)), 1)


def test_rows_block_under_fused_0_in_a_child_process():
    env = {k: v for k, v in os.environ.items() if k != "MI355ASR_SMALL_M"}
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "rows_block"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=120, env=dict(env, MI355ASR_FUSED="0"))
    print(r.stdout)
    assert r.returncode == 0, "exit status %d\n%s" % (r.returncode, r.stdout[-4000:])
    assert "step rows_block ok" in r.stdout


# ---- (b), (c) the single-stream calls -----------------------------------------------------------------------------------------
def test_single_stream_picker_packet():
    """one packet of 16 mel frames -> 4 rows through front, encoder and picker"""
    from caller_contract_gpu_steps import profile_counts
    m, x, cfg = chunk_case()
    call = lambda: picker_packet(m, x)
    assert call()[0].shape[1] == 4
    assert_counts("picker_stream_predict", profile_counts(m._h, call), cfg["enc_num_blocks"] + cfg["picker_num_blocks"],
                  CTC_PROJECT=1, CTC_HEAD=1, **FRONT)
    assert_same_bits("picker_stream_predict", call(), call())


def test_single_stream_decoder_on_the_picked_rows():
    from caller_contract_gpu_steps import profile_counts
    m, x, cfg = chunk_case()
    vp, _, vh, _ = picker_packet(m, x)
    f, _ = m.feature_pick(vh, vp)
    assert f.shape[1] == 4                                    # every frame picked
    call = lambda: m.decoder_stream_predict(f, m.init_decoder_caches(1))
    assert_counts("decoder_stream_predict", profile_counts(m._h, call), cfg["helper_num_blocks"] + cfg["decoder_num_blocks"],
                  CTC_PROJECT=1, CTC_HEAD=1)
    assert_same_bits("decoder_stream_predict", call(), call())


# ---- (d) the batched streams ----------------------------------------------------------------------------------------------------
def test_stream_step_of_two_slots_at_different_ages():
    """slot 0 reset, slot 1 one packet old: the per-stream row tables of the tick differ"""
    from caller_contract_gpu_steps import profile_counts
    from test_gpu_chunk_streams import W
    m, x, cfg = chunk_case()
    st = m.open_streams(2)
    m.stream_step(st, [1], [x[1][:W]])
    m.reset_streams(st, [0])
    saved = st.buf.clone()

    def call():
        st.buf.copy_(saved)
        return m.stream_step(st, [0, 1], [x[0][:W], x[1][W:2 * W]], want_logits=True)

    blocks = sum(cfg[k + "_num_blocks"] for k in ("enc", "picker", "helper", "decoder"))
    assert_counts("stream_step", profile_counts(m._h, call), blocks, CTC_PROJECT=2, CTC_HEAD=2, **FRONT)
    r0, r1 = call(), call()
    assert r0[0]["n_picked"] == 4 and r0[1]["n_picked"] == 4
    assert_same_bits("stream_step", r0, r1)


if __name__ == "__main__":
    import torch
    for p in (os.path.dirname(HERE), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    assert torch.cuda.is_available(), "needs cuda:0 (MI355X)"
    name = sys.argv[1]
    globals()["step_" + name]()
    torch.cuda.synchronize()
    print("step %s ok" % name)
