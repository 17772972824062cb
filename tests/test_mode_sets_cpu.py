"""The derived mode tuples of feddat_amd.modes and mode_names on one fixed key list (no GPU, no library)."""
from feddat_amd.modes import ADAPTERLESS_MODES, MODES, PROMPT_MODE, SINGLE_PASS_MODES, VECTOR_MODES, mode_names

E = "vilt_encoder.vilt."
TXT_LN_W = E + "embeddings.text_embeddings.LayerNorm.weight"
TXT_LN_B = E + "embeddings.text_embeddings.LayerNorm.bias"
PATCH_B = E + "embeddings.patch_embeddings.projection.bias"
PR_VIS = E + "embeddings.prompt_embedding_vis.0.weight"
PR_TEXT_B = E + "embeddings.prompt_embedding_text.1.bias"
Q_W = E + "encoder.layer.0.attention.attention.query.weight"
Q_B = E + "encoder.layer.0.attention.attention.query.bias"
LN1_W = E + "encoder.layer.0.layernorm_before.weight"
LN1_B = E + "encoder.layer.0.layernorm_before.bias"
AD_W = E + "encoder.layer.0.output.adapter.adapter_down.weight"
AD0_W = E + "encoder.layer.0.output.adapter.adapter_0_down.weight"
AD1_B = E + "encoder.layer.0.output.adapter.adapter_1_up.bias"
AD2_W = E + "encoder.layer.0.output.adapter.adapter_2_up.weight"
LNF_W = E + "layernorm.weight"
POOL_B = E + "pooler.dense.bias"
FC0_B = "task_layer.art.clf_fc0.bias"
NORM0_W = "task_layer.art.clf_norm0.weight"
LM_B = "text_decoder.cls.predictions.bias"
KEYS = [TXT_LN_W, TXT_LN_B, PATCH_B, PR_VIS, PR_TEXT_B, Q_W, Q_B, LN1_W, LN1_B, AD_W, AD0_W, AD1_B, AD2_W, LNF_W, POOL_B, FC0_B,
        NORM0_W, LM_B]

# what mode_names returned for KEYS before the tuples below existed
EXPECTED = {
    "dat": dict(trainable=[AD0_W, AD1_B, FC0_B, NORM0_W, LM_B], communicated=[AD1_B],
                personal=[AD0_W, AD2_W, FC0_B, NORM0_W, LM_B]),
    "adapter": dict(trainable=[AD_W, AD0_W, AD1_B, AD2_W, FC0_B, NORM0_W], communicated=[AD_W, AD0_W, AD1_B, AD2_W],
                    personal=[FC0_B, NORM0_W]),
    "bias": dict(trainable=[TXT_LN_B, PATCH_B, PR_TEXT_B, Q_B, LN1_B, AD1_B, POOL_B, FC0_B, NORM0_W, LM_B],
                 communicated=[TXT_LN_B, PATCH_B, PR_TEXT_B, Q_B, LN1_B, AD1_B, POOL_B, FC0_B, LM_B],
                 personal=[FC0_B, NORM0_W]),
    "norm": dict(trainable=[LN1_W, LN1_B, LNF_W, FC0_B, NORM0_W], communicated=[LN1_W, LN1_B, LNF_W, NORM0_W],
                 personal=[FC0_B, NORM0_W]),
    "prompt": dict(trainable=[PR_VIS, PR_TEXT_B, FC0_B, NORM0_W], communicated=[PR_VIS, PR_TEXT_B], personal=[FC0_B, NORM0_W]),
}


def test_derived_tuples_partition_the_modes():
    every = MODES + (PROMPT_MODE,)
    assert ADAPTERLESS_MODES == VECTOR_MODES + (PROMPT_MODE,) == ("bias", "norm", "prompt")
    assert SINGLE_PASS_MODES == ("adapter",) + ADAPTERLESS_MODES
    assert len(set(every)) == len(every) == 5
    # dat | single-pass is every mode, each once; adapter | adapter-less is the single-pass modes, each once
    assert sorted(("dat",) + SINGLE_PASS_MODES) == sorted(every)
    assert "dat" not in SINGLE_PASS_MODES and "dat" not in ADAPTERLESS_MODES
    assert "adapter" in SINGLE_PASS_MODES and "adapter" not in ADAPTERLESS_MODES


def test_mode_names_on_a_fixed_key_list():
    assert sorted(EXPECTED) == sorted(MODES + (PROMPT_MODE,))
    for mode, want in EXPECTED.items():
        assert mode_names(KEYS, mode) == want, mode
