"""A single sequence is ONE ROW of the device sampler's row kernels (csrc/sampler.hip: enqueue_rows): l2_decode_sample launches the same
kernels as l2_decode_sample_batch, at one row, with the picker of its mode chosen on the host and the maximum taken from the classifier's
argmax keys.  The same seeded run made four ways -- through the library's queue (the sampler's recorder), through replayed hipGraphs,
eagerly, and as row 0 of a one-row batch (the sampler's own max pass, every picker launched) -- gives the same tokens and the same rng
state.  Vocabularies: 1000 (one ragged tile), 5121 (a tile holding one element; sort tiles and sum tiles both ragged), 50257 (seven groups
of the rank merge, the last one ragged).  Bit-equality is exact by construction: no tolerance."""
import pytest

from llama2_ts_amd import runtime

pytestmark = pytest.mark.gpu
STEPS, SEED = 24, 20261018
SETTINGS = ((0.9, 1.0), (0.9, 0.9))      # plain sample, top-p


def single(hdr, options, queue):
    ctx = runtime.Context(hdr)
    ctx.synth_fill(3)
    for key, value in options:
        ctx.set_option(key, value)
    runs = [ctx.decode_sample(1, 0, STEPS, t, p, SEED) for t, p in SETTINGS]
    assert ctx.get_option(runtime.OPT_AQL_QUEUE) == queue, ctx.dispatch_reason()
    assert ctx.get_option(runtime.OPT_SAMPLED_TOKENS) == STEPS * len(SETTINGS)
    ctx.close()
    return [(toks.tolist(), rng) for toks, rng in runs]


def one_row_batch(hdr):
    ctx = runtime.Context(hdr)
    ctx.synth_fill(3)
    ctx.seq_reserve(1)
    runs = [ctx.decode_sample_batch([0], [1], [0], STEPS, t, p, [SEED]) for t, p in SETTINGS]
    assert ctx.get_option(runtime.OPT_BATCH_SAMPLED_TOKENS) == STEPS * len(SETTINGS)
    ctx.close()
    return [(toks[0].tolist(), int(rng[0])) for toks, rng in runs]


@pytest.mark.parametrize("vocab", [1000, 5121, 50257])
def test_one_row_four_ways(vocab):
    hdr = (64, 176, 2, 4, 4, vocab, 64)
    runs = {"queue": single(hdr, (), 1),
            "graph": single(hdr, ((runtime.OPT_AQL_QUEUE, 0),), 0),
            "eager": single(hdr, ((runtime.OPT_USE_GRAPH, 0),), 0),
            "batch row": one_row_batch(hdr)}
    for way, got in runs.items():
        print(vocab, way, got)
    for way, got in runs.items():
        assert got == runs["queue"], (vocab, way)
