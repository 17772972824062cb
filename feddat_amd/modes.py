"""Which state-dict tensors train, travel to the server and stay with the client, per optimizer_mode (src/train/main.py:
114-118,141-163,176-196,246-250 and the personal-parameter shuttle of main.py:440-450,467-497).  The reference matches by
case-sensitive SUBSTRING, over named_parameters() for "trainable" and over state_dict() keys for "communicated", and this
module does the same on the keys it is given.

  mode       trainable                      communicated (FedAvg)     personal (kept per client)
  dat        adapter_0, adapter_1, heads    adapter_1                 heads, adapter_0, adapter_2
             (heads: ViLT's task_layer.* ('task'); ALBEF's text_decoder.cls.predictions.* ('.cls.'), present in an ALBEF state dict
             only when the model was built with train_lm_head=True)
  adapter    adapter, heads                 every 'adapter' key       heads ('task'; albef=True: '.cls.' too)
  bias       every 'bias' key, heads        every 'bias' key          heads ('task')
  norm       every 'norm' key, heads        every 'norm' key          heads ('task')
  prompt     every 'prompt' key, heads      every 'prompt' key        heads ('task')

prompt (main.py:198-245): embeddings.prompt_embedding_{vis,text}.{0.weight, 1.weight, 1.bias, 3.weight, 3.bias}, 299 712 floats
per module, 599 424 communicated.  The forward reads the text module on both sides of the sequence (prompted_output.py:254), so
the vis tensors are trainable by name but never get a gradient: AdamW skips them and they travel unchanged.  No 'prompt' key
contains 'clf'.  prompt_engine.ViltPromptEngine runs the mode; the command line (train.main) does not offer it yet, which is why
it is PROMPT_MODE beside MODES and not a fifth entry of it.

bias (BitFit): per layer query|key|value.bias, attention.output.dense.bias, intermediate.dense.bias, output.dense.bias (the HF key: no Adaptered_ViltOutput here),
layernorm_before.bias, layernorm_after.bias (8 448 floats), once text_embeddings.LayerNorm.bias,
patch_embeddings.projection.bias, layernorm.bias, pooler.dense.bias: 104 448 backbone floats at 12 layers.
norm: layernorm_before.{weight,bias}, layernorm_after.{weight,bias}, vilt.layernorm.{weight,bias} (38 400 floats).
text_embeddings.LayerNorm.* does NOT match 'norm' (capital N) and stays frozen.

Tensors that are BOTH communicated and personal: the heads' own matches -- task_layer.<t>.clf_fc0.bias, clf_norm0.bias and
clf_fc1.bias in bias mode; task_layer.<t>.clf_norm0.weight and clf_norm0.bias in norm mode (the head's LayerNorm is named
clf_norm0: vilt.py:202-209).  They sit in the server's comm_state_dict_names, but get_average_net skips every key that
contains 'clf' (main.py:54), and each client overwrites them with its personal copy before it trains (main.py:467-474):
the server's copies never move, the clients' never mix.  averaged_names() is the communicated list minus those keys, i.e.
what actually changes on the server.

Weight decay follows task_trainer.py:477-504 (local_update._no_decay): a name containing 'bias' or 'LayerNorm.weight' is
not decayed.  layernorm_{before,after}.weight and vilt.layernorm.weight contain neither, so the gammas of norm mode ARE
decayed; every bias is not.
"""
from __future__ import annotations

from typing import Dict, List, Sequence

from . import lib as L

MODES = ("dat", "adapter", "bias", "norm")
# the modes whose trainable backbone tensors are per-column vectors (vector_engine.ViltVectorEngine)
VECTOR_MODES = ("bias", "norm")
# prompt tuning (prompt_engine.ViltPromptEngine): known to mode_names / averaged_names and the Python surface, not to train.main
PROMPT_MODE = "prompt"
# the modes with no adapter in the backbone (single_pass.ViltFrozenEngine), and the modes that run the reference's non-dat
# train_step, one pass per batch (single_pass.SinglePassStep): every mode but dat
ADAPTERLESS_MODES = VECTOR_MODES + (PROMPT_MODE,)
SINGLE_PASS_MODES = ("adapter",) + ADAPTERLESS_MODES


def mode_names(keys: Sequence[str], mode: str, albef: bool = False) -> Dict[str, List[str]]:
    """{"trainable", "communicated", "personal"}: the subsets of `keys` (state-dict order kept) for optimizer_mode `mode`.
    albef: the keys are an ALBEF model's (encoder_name albef*): in the non-dat modes its LM head ('.cls.') trains and is personal
    too, as main.py:127-128,247-250 has it; dat treats '.cls.' that way on any key list."""
    if mode not in MODES + (PROMPT_MODE,):
        raise L.FeddatHipError(f"optimizer_mode must be one of {MODES + (PROMPT_MODE,)}, got {mode!r}")
    keys = list(keys)
    if mode == "dat":
        # '.cls.': the ALBEF decoder's LM head (main.py:127-128,247-250); no ViLT key contains it
        return dict(trainable=[k for k in keys if "task" in k or ".cls." in k or "adapter_0" in k or "adapter_1" in k],
                    communicated=[k for k in keys if "adapter_1" in k],
                    personal=[k for k in keys if "task" in k or ".cls." in k or "adapter_0" in k or "adapter_2" in k])
    sub = mode          # "adapter" | "bias" | "norm" | "prompt": the substring main.py matches is the mode's own name
    # the heads: 'task' (ViLT); with albef=True '.cls.' as well, the decoder's LM head, trainable and personal where the encoder
    # is ALBEF (main.py:127-128,247-250)
    head = (lambda k: "task" in k or ".cls." in k) if albef else (lambda k: "task" in k)
    return dict(trainable=[k for k in keys if sub in k or head(k)],
                communicated=[k for k in keys if sub in k],
                personal=[k for k in keys if head(k)])


def averaged_names(keys: Sequence[str], mode: str) -> List[str]:
    """The communicated keys the server really averages: get_average_net leaves out every key containing 'clf' (main.py:54)."""
    return [k for k in mode_names(keys, mode)["communicated"] if "clf" not in k]
