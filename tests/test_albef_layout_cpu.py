"""Where the ALBEF engine's pieces live: the frozen model and forward in albef_backbone, the evaluation in albef_rank, the
backward and the step in albef_engine -- and everything callers import from feddat_amd.albef_engine still there.  Needs no
library and no device."""
from feddat_amd import albef_backbone, albef_engine, albef_rank
from feddat_amd.local_update import LocalUpdateEngine

E = albef_engine.AlbefDatEngine


def _home(name):
    """Module of the class in E's MRO that defines `name`."""
    owner = next(c for c in E.__mro__ if name in c.__dict__)
    return owner.__module__.rsplit(".", 1)[-1]


def test_names_callers_use_import_from_albef_engine():
    for name in ("AlbefDatEngine", "rank_slab_plan", "slab_question_of_row", "lm_head_group_spec", "PRE", "LM_HEAD", "ADAPTER_TENSORS"):
        assert hasattr(albef_engine, name), name
    assert albef_engine.rank_slab_plan is albef_rank.rank_slab_plan
    assert albef_engine.slab_question_of_row is albef_rank.slab_question_of_row
    assert albef_engine.lm_head_group_spec is albef_backbone.lm_head_group_spec
    assert albef_engine.PRE == "albef_model.albef." and albef_engine.LM_HEAD == albef_engine.PRE + "text_decoder.cls.predictions."
    assert albef_engine.ADAPTER_TENSORS == ("down.weight", "down.bias", "up.weight", "up.bias")
    for name in ("train_step", "begin_local_update", "set_batch", "state_dict", "load_tensors", "repack", "rank_answer",
                 "forward_train_logits", "image_embeds", "scaler_state", "assert_finite", "_capture", "_named_groups", "_rank_maps",
                 "_drop"):
        assert callable(getattr(E, name)), name


def test_engine_derives_from_backbone_and_local_update_engine():
    assert issubclass(E, albef_backbone.AlbefBackbone) and issubclass(E, LocalUpdateEngine)
    assert issubclass(E, albef_rank.AlbefRank)
    assert issubclass(albef_backbone.AlbefBackbone, LocalUpdateEngine)
    # the evaluation needs nothing of the backward or the step: the mixin stands beside the backbone, not on the engine
    assert not issubclass(albef_rank.AlbefRank, LocalUpdateEngine)
    mro = E.__mro__
    assert mro.index(albef_rank.AlbefRank) < mro.index(albef_backbone.AlbefBackbone) < mro.index(LocalUpdateEngine)


def test_each_role_is_defined_in_its_module():
    for name in ("forward_train_logits", "rank_answer", "_rank_maps", "_rank_answer_slabs", "_rank_answer_frame", "_as_mode"):
        assert _home(name) == "albef_rank", name
    for name in ("set_batch", "repack_adapter", "_segs", "_vit_fwd", "_embed", "_dense_resid", "_attn_out", "_bert_fwd", "_forward",
                 "_forward_text", "_text_questions", "_text_answers", "_lm_head_fwd", "_drop", "image_embeds", "_stage_questions"):
        assert _home(name) == "albef_backbone", name
    for name in ("__init__", "_bert_bwd", "_vit_bwd", "_backward", "_backward_text", "_lm_head_bwd", "_towers_bwd", "_wgrad",
                 "_wgrad_reduce", "_scale_in", "_alloc_head_grads", "_head_step_a", "_forward_stacked", "_forward_two_passes",
                 "_image_bwd_stacked", "_step_kernels_head", "_step_kernels", "begin_local_update", "_capture", "load_tensors",
                 "repack"):
        assert _home(name) == "albef_engine", name
    assert _home("train_step") == "local_update"


def test_one_segment_list_per_mode():
    seg = albef_backbone.AlbefBackbone._mode_segments
    assert seg("gating", 10) == [(0, 10, [(0, 0.5), (2, 0.5)])]
    assert seg("adapter_1", 10) == [(0, 10, [(1, 1.0)])] and seg("adapter_0", 7) == [(0, 7, [(0, 1.0)])]
    assert seg("both", 10) == [(0, 5, [(0, 0.5), (2, 0.5)]), (5, 10, [(1, 1.0)])]
