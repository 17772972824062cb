"""Drop-in mirrors of the reference's module API for the hot path, backed by libfeddat_hip.so.

  reference                                              here
  src/modeling/models/adapter.py        Adapter                   -> Adapter
  src/modeling/adaptered_output.py      Adaptered_ViltOutput      -> Adaptered_ViltOutput
  src/modeling/vilt.py                  ViltContinualLearner      -> ViltContinualLearner (create_vilt_continual_learner_model)

Same names, same call signatures, same mode-switch semantics (including the requires_grad side effects of
set_active_adapter that decide optimizer membership, adapter.py:66-95).  Tensors are device tensors; every forward
is a HIP kernel launch through the C ABI -- there is no PyTorch arithmetic and no CPU path (a missing library or a
CPU tensor raises FeddatHipError).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import torch

from . import lib as L
from .engine import ViltDatEngine, ENC
from .modes import ADAPTERLESS_MODES, MODES, PROMPT_MODE, SINGLE_PASS_MODES, VECTOR_MODES, mode_names


class _Param:
    """Minimal stand-in for nn.Parameter: .data is a device tensor (a view into an engine buffer or an own
    allocation), .requires_grad is the flag the reference toggles."""

    def __init__(self, data: torch.Tensor, requires_grad: bool = True):
        self.data = data
        self.requires_grad = requires_grad

    @property
    def shape(self):
        return self.data.shape


class _Linear:
    def __init__(self, weight: torch.Tensor, bias: torch.Tensor):
        self.weight = _Param(weight)
        self.bias = _Param(bias)

    def parameters(self):
        return [self.weight, self.bias]


class Adapter:
    """adapter.py:16-163.  Bottleneck adapters `adapter_{i}_{down,up}` (model_dim -> model_dim/16 -> model_dim,
    ReLU); forward(hidden_states, input_tensor) in single-adapter or fixed 0.5/0.5 "gating" mode."""

    def __init__(self, names, device, model_dim: int = 768, adapter_reduction_factor: int = 16, _views=None):
        L.load()
        if model_dim != 768 or adapter_reduction_factor != 16:
            raise L.FeddatHipError("the HIP adapter kernel is specialised for model_dim=768, reduction=16 "
                                   "(the only configuration the reference ever instantiates, adapter.py:22)")
        self.actv = "relu"
        self.scaling = 1.0
        self.gating = False
        if isinstance(names, str):
            names = [names]
        self.names = [n for n in names if "adapter" in n]
        self.device = torch.device(device)
        r = model_dim // adapter_reduction_factor
        # the module belongs to the operand format (library) the constructing thread is bound to: lib.operands(...)
        self._fmt = L.current_operands()
        op = L.OPERAND_DTYPE[self._fmt]
        self._packs: Dict[str, dict] = {}
        for n in self.names:
            if _views is not None:
                wd, bd, wu, bu = _views[n]
            else:  # init_bert_weights: N(0, 0.02) weights, zero biases (adapter.py:5-14)
                wd = torch.randn(r, model_dim, device=self.device) * 0.02
                bd = torch.zeros(r, device=self.device)
                wu = torch.randn(model_dim, r, device=self.device) * 0.02
                bu = torch.zeros(model_dim, device=self.device)
            setattr(self, f"{n}_down", _Linear(wd, bd))
            setattr(self, f"{n}_up", _Linear(wu, bu))
            self._packs[n] = dict(
                wd=torch.empty(r, model_dim, dtype=op, device=self.device),
                wdT=torch.empty(model_dim, r, dtype=op, device=self.device),
                wu=torch.empty(model_dim, r, dtype=op, device=self.device),
                wuT=torch.empty(r, model_dim, dtype=op, device=self.device), bd=bd, bu=bu)
        if hasattr(self, "adapter_2_down"):                      # adapter.py:55-58
            for m in (self.adapter_2_down, self.adapter_2_up):
                for p in m.parameters():
                    p.requires_grad = False
        self.refresh()

    def refresh(self):
        """Re-derive the 16-bit operand copies after the fp32 weights changed."""
        with L.operands(self._fmt):
            for n, p in self._packs.items():
                L.adapter_pack(getattr(self, f"{n}_down").weight.data, getattr(self, f"{n}_up").weight.data, p["wd"],
                               p["wdT"], p["wu"], p["wuT"])

    def deactivate_gating(self):
        self.gating = False

    def activate_gating(self):
        self.gating = True

    def set_active_adapter(self, name):                           # adapter.py:66-95
        if isinstance(name, str):
            self.active_adapter_down = getattr(self, f"{name}_down")
            self.active_adapter_up = getattr(self, f"{name}_up")
            self._active = name

        def flag(n, v):
            for m in (getattr(self, f"{n}_down"), getattr(self, f"{n}_up")):
                for p in m.parameters():
                    p.requires_grad = v
        if name == "adapter_0":
            flag("adapter_0", True)
            flag("adapter_1", False)
        elif name == "adapter_1":
            flag("adapter_1", True)
            flag("adapter_0", False)
        elif isinstance(name, list):
            for n in name:
                flag(n, True)

    def named_parameters(self):
        for n in self.names:
            for part in ("down", "up"):
                lin = getattr(self, f"{n}_{part}")
                yield f"{n}_{part}.weight", lin.weight
                yield f"{n}_{part}.bias", lin.bias

    def forward(self, hidden_states: torch.Tensor, input_tensor: torch.Tensor) -> torch.Tensor:
        """adapter.py:124-163.  The reference always calls adapter(h, h) (adaptered_output.py:77); the fused kernel
        implements exactly that form, so a distinct input_tensor is rejected loudly."""
        if hidden_states.data_ptr() != input_tensor.data_ptr():
            raise L.FeddatHipError("fused adapter kernel requires input_tensor is hidden_states "
                                   "(adaptered_output.py:77 is the only call site)")
        x = hidden_states
        if x.dtype != torch.float32 or not x.is_contiguous():
            raise L.FeddatHipError("adapter forward expects a contiguous fp32 device tensor [..., 768]")
        T = x.numel() // 768
        if not self.gating:
            ads = [dict(self._packs[self._active], scale=1.0)]
        elif hasattr(self, "adapter_2_down"):
            ads = [dict(self._packs["adapter_0"], scale=0.5 * self.scaling),
                   dict(self._packs["adapter_2"], scale=0.5 * self.scaling)]
        else:
            ads = [dict(self._packs["adapter_0"], scale=0.5 * self.scaling),
                   dict(self._packs["adapter_1"], scale=0.5 * self.scaling)]
        out = torch.empty_like(x)
        with L.operands(self._fmt):
            L.adapter_fwd(x.view(T, 768), out.view(T, 768), L.make_segs([dict(row_begin=0, row_end=T, adapters=ads)]), T)
        return out

    __call__ = forward


class Adaptered_ViltOutput:
    """adaptered_output.py:67-78: h = dense(x) (+ dropout p=0) + input_tensor; return adapter(h, h).
    `layer` supplies the frozen ViltOutput dense as .dense.weight [768,3072] / .dense.bias [768] device tensors."""

    def __init__(self, layer, adapter_config) -> None:
        self.layer = layer
        self.adapter = Adapter(**adapter_config, model_dim=768)
        w = layer.dense.weight.data if hasattr(layer.dense.weight, "data") else layer.dense.weight
        self._fmt = self.adapter._fmt
        self._w16 = torch.empty(w.shape, dtype=L.OPERAND_DTYPE[self._fmt], device=w.device)
        with L.operands(self._fmt):
            L.cvt_f32_bf16(w.contiguous().float(), self._w16)
        b = layer.dense.bias
        self._b = (b.data if hasattr(b, "data") else b).contiguous().float()

    def forward(self, hidden_states: torch.Tensor, input_tensor: torch.Tensor) -> torch.Tensor:
        x = hidden_states.reshape(-1, hidden_states.shape[-1])
        res = input_tensor.reshape(-1, 768).contiguous().float()
        h = torch.empty_like(res)
        with L.operands(self._fmt):
            if x.dtype != self._w16.dtype:
                x16 = torch.empty(x.shape, dtype=self._w16.dtype, device=x.device)
                L.cvt_f32_bf16(x.contiguous().float(), x16)
                x = x16
            L.gemm_bf16_nt(x, self._w16, L.EPI_RESID_F32, bias=self._b, resid=res, out_f32=h)
        return self.adapter(h, h).view(input_tensor.shape)

    __call__ = forward


class ViltContinualLearner:
    """vilt.py:154-382 for the classification / single-image path, on the HIP engine.

    forward(task_key, images, texts) -> (pooled, logits) takes the reference's batch schema: `images` = list of decoded
    RGB images ([H, W, 3] uint8 arrays / tensors, or PIL images), `texts` = list of questions (vilt.py:244-264); they go
    through process_inputs -- the device image processor + device WordPiece tokenizer, ONCE per batch (the reference runs
    its host processor inside every one of the three forward passes of a train_step).  A ready-made HF ViLT encodings
    dict (pixel_values, pixel_mask, input_ids, attention_mask, token_type_ids) in `images` with texts=None is taken as is
    (the golden harness and the synthetic benchmarks feed tensors).

    vocab: path of the BERT vocab.txt (the reference loads ./models/bert-base-uncased, vilt.py:47-48) or the token list."""

    BERT_LOCAL_PATH = "./models/bert-base-uncased"       # vilt.py:47

    def __init__(self, ordered_cl_tasks: List[str], params: Dict[str, torch.Tensor], device, batch_size: int,
                 image_size=384, num_layers: int = 12, lr: float = 1e-4, vocab=None, operands: str = None,
                 optimizer_mode: str = "dat", num_labels: int = 100, max_patches: Optional[int] = None,
                 dataset_resize: bool = False):
        """dataset_resize: images whose shorter side exceeds 384 pass the image datasets' bilinear Resize(384, max_size=640)
        before the processor, as the reference's datasets do (cocoimages_dataset_crossvqas.py:83,108-109; on the device,
        image_processing.DatasetResize).  Off by default: images reach the processor as they are given.
        image_size: the engine's static pixel frame, an int (square) or (height, width).
        max_patches: patch slots per sample instead of one sequence position per cell of the frame (ViltBackbone): with
        image_size=(640, 640), max_patches=240 one engine takes every image the ViLT size rule yields, portrait and landscape.
        num_labels: width of every task head (task_configs_fed.py: 100 for the CLOVE / domain tasks, 3129 for vqa; one engine
        has one width).
        operands: 16-bit MFMA operand format of the engine, "f16" (default; the reference's mixed_precision: fp16,
        accelerate_config.yaml:8) or "bf16" (engine.ViltDatEngine).
        optimizer_mode: "dat" (adapter_{0,1,2}, engine.ViltDatEngine) or "adapter" (the FedAvg baseline: one adapter per
        layer, adapter_engine.ViltAdapterEngine; main.py:114-118,141-149), "bias" or "norm" (the plain backbone with every
        'bias' / 'norm' parameter trainable, vector_engine.ViltVectorEngine; main.py:176-196), or "prompt" (the plain backbone
        with the reference's two prompt modules, prompt_engine.ViltPromptEngine; main.py:198-245).  state_dict() holds the
        trainable tensors under the reference's keys; bias / norm add no parameters."""
        self.ordered_cl_tasks = list(ordered_cl_tasks)
        self.device = torch.device(device)
        self.optimizer_mode = optimizer_mode
        if optimizer_mode == "adapter":
            from .adapter_engine import ViltAdapterEngine as Engine
        elif optimizer_mode == "dat":
            Engine = ViltDatEngine
        elif optimizer_mode in VECTOR_MODES:
            from .vector_engine import ViltVectorEngine as Engine
        elif optimizer_mode == PROMPT_MODE:
            from .prompt_engine import ViltPromptEngine as Engine
        else:
            raise L.FeddatHipError(f"optimizer_mode must be one of {MODES + (PROMPT_MODE,)}, got {optimizer_mode!r}")
        self.engine = Engine(params, self.ordered_cl_tasks, self.device, batch=batch_size, res=image_size, layers=num_layers,
                             lr=lr, operands=operands, num_labels=num_labels,
                             **({"mode": optimizer_mode} if optimizer_mode in ADAPTERLESS_MODES else {}),
                             **({} if max_patches is None else {"max_patches": max_patches}))
        self.num_labels = int(num_labels)
        self.max_text_length = self.engine.Lt               # vilt.py:50: config.max_position_embeddings = 40
        self._vocab = vocab
        self._tokenizer = None
        self._image_processor = None
        self.dataset_resize, self._dataset_resize = bool(dataset_resize), None
        self.gating = False
        self.active = "adapter_1" if optimizer_mode == "dat" else "adapter" if optimizer_mode == "adapter" else None
        # requires_grad flags per adapter, toggled exactly like adapter.py:66-95; prepare_model's initial state
        # (main.py:157-159 + adapter.py:55-58): adapter_0/1 trainable, adapter_2 frozen.  The single adapter is always
        # trainable (set_active_adapter('adapter') flips no flag)
        self.adapter_requires_grad = {0: True, 1: True, 2: False} if optimizer_mode == "dat" else \
            {0: True} if optimizer_mode == "adapter" else {}
        # main.py:141-149,160-163,176-196: adapter_1 (dat) / every adapter key (adapter) / every 'bias' resp. 'norm' key
        self.comm_state_dict_names = mode_names(list(self.state_dict()), optimizer_mode)["communicated"]

    # ---- adapter switches (vilt.py:363-373) ----
    def set_active_adapter(self, name):
        if self.optimizer_mode in ADAPTERLESS_MODES:
            raise L.FeddatHipError(f"optimizer_mode {self.optimizer_mode} has no adapter (got {name!r})")
        if self.optimizer_mode == "adapter":
            if name != "adapter":
                raise L.FeddatHipError(f"optimizer_mode adapter has one adapter, 'adapter' (got {name!r})")
            return
        self.active = name
        if name == "adapter_0":
            self.adapter_requires_grad[0], self.adapter_requires_grad[1] = True, False
        elif name == "adapter_1":
            self.adapter_requires_grad[1], self.adapter_requires_grad[0] = True, False

    def activate_gating(self):
        self.gating = True

    def deactivate_gating(self):
        self.gating = False

    def optimizer_adapters(self) -> Sequence[int]:
        """Which adapters a freshly created optimizer would hold (create_optimizer filters on requires_grad)."""
        if self.optimizer_mode == "adapter":
            return (0,)
        if self.optimizer_mode in ADAPTERLESS_MODES:      # no adapter: the optimizer holds the mode's tensors and the head
            return ()
        return tuple(a for a in (0, 1) if self.adapter_requires_grad[a])

    # ---- state dict with the reference's keys ----
    def state_dict(self) -> Dict[str, torch.Tensor]:
        return self.engine.state_dict()

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = False):
        own = self.engine.state_dict()
        unknown = [k for k in sd if k not in own]
        if strict and unknown:
            raise KeyError(f"unexpected keys: {unknown[:3]}")
        self.engine.load_tensors({k: v for k, v in sd.items() if k in own})

    def after_load(self):
        self.engine.repack()

    # ---- the reference's batch schema (vilt.py:87-100): images + questions -> HF ViLT encodings, on the device ----
    @property
    def tokenizer(self):
        if self._tokenizer is None:
            import os
            from .tokenization import WordPieceTokenizer
            vocab = self._vocab
            if vocab is None:
                vocab = os.path.join(self.BERT_LOCAL_PATH, "vocab.txt")
                if not os.path.exists(vocab):
                    raise L.FeddatHipError(
                        f"texts were given but there is no BERT vocabulary: pass vocab=<vocab.txt path or token list> to "
                        f"ViltContinualLearner, or place bert-base-uncased at {self.BERT_LOCAL_PATH} as the reference does")
            self._tokenizer = WordPieceTokenizer(vocab, self.device)
        return self._tokenizer

    @property
    def image_processor(self):
        if self._image_processor is None:
            from .image_processing import ViltImageProcessor
            # every batch is padded to the engine's static frame; patches outside an image's valid rectangle are masked keys
            # (grid frame) or stay out of the sequence (patch slots)
            self._image_processor = ViltImageProcessor(self.device, pad_to=self.engine.res)
        return self._image_processor

    def process_inputs(self, images: List, texts: List[str]) -> Dict[str, torch.Tensor]:
        """ViltEncoderWrapper.process_inputs (vilt.py:87-100): ViltProcessor(images, text, max_length=40, padding=True,
        truncation=True) -> {pixel_values, pixel_mask, input_ids, attention_mask, token_type_ids}, as device tensors in the
        engine's static frame: images resized by the ViLT rule (shorter edge 384, longer <= 640, multiples of 32) and
        zero-padded to the frame with their pixel_mask, questions padded to max_text_length with attention_mask 0 -- the
        pooled feature does not depend on how far a batch is padded (masked keys; golden G6)."""
        import numpy as np
        arrs = [np.asarray(im.convert("RGB")) if hasattr(im, "convert") else im for im in images]
        if len(arrs) != len(texts):
            raise L.FeddatHipError(f"{len(arrs)} images but {len(texts)} texts")
        eng = self.engine
        stage1 = None
        if self.dataset_resize:      # the datasets' Resize first: the slot budget below and the processor's frame check see
            from .image_processing import DatasetResize, decoded_images      # the sizes it leaves
            if self._dataset_resize is None:
                self._dataset_resize = DatasetResize(self.device)
            stage1, arrs = self._dataset_resize, decoded_images(arrs)
            sizes = [stage1.output_size(a.shape[0], a.shape[1], larger_only=True) for a in arrs]
        if eng.max_patches is not None:      # the slot budget, from the sizes alone (before any image is resized)
            from .image_processing import resize_output_size
            for i, a in enumerate(arrs):
                shp = a.shape if hasattr(a, "shape") else None
                if stage1 is not None:
                    shp = sizes[i] + (3,)
                if shp is not None and len(shp) == 3:
                    oh, ow = resize_output_size(int(shp[0]), int(shp[1]))
                    if (oh // eng.P) * (ow // eng.P) > eng.max_patches:
                        raise L.FeddatHipError(f"image {i} ({shp[0]}x{shp[1]}) resizes to {oh}x{ow}: {(oh // eng.P) * (ow // eng.P)} "
                                               f"patches, the engine was built with max_patches = {eng.max_patches}")
        enc = dict(self.image_processor(arrs if stage1 is None else stage1(arrs, larger_only=True)))
        tok = self.tokenizer(list(texts), padding="max_length", truncation=True, max_length=self.max_text_length)
        enc.update(input_ids=tok["input_ids"], attention_mask=tok["attention_mask"], token_type_ids=tok["token_type_ids"])
        return enc

    def forward(self, task_key: str, images, texts=None):
        if not isinstance(images, dict):
            images = self.process_inputs(images, texts)
        if self.optimizer_mode in SINGLE_PASS_MODES:
            return self.engine.forward(images, task_key)
        mode = "gating" if self.gating else self.active
        return self.engine.forward(images, mode, task_key)

    __call__ = forward


def create_vilt_continual_learner_model(params: Dict[str, torch.Tensor], ordered_cl_tasks: List[str], device,
                                        batch_size: int, image_size=384, num_layers: int = 12,
                                        lr: float = 1e-4, vocab=None, operands: str = None,
                                        optimizer_mode: str = "dat", num_labels: int = 100,
                                        max_patches: Optional[int] = None,
                                        dataset_resize: bool = False) -> ViltContinualLearner:
    """vilt.py:421-452 (the pretrained checkpoint is passed in as a tensor dict: feddat_amd.weights.load_vilt_pretrained
    reads it from a local HF directory; there is no hub access here)."""
    return ViltContinualLearner(ordered_cl_tasks, params, device, batch_size, image_size, num_layers, lr, vocab=vocab,
                                operands=operands, optimizer_mode=optimizer_mode, num_labels=num_labels,
                                max_patches=max_patches, dataset_resize=dataset_resize)


def convert_batch_to_vilt_input_dict(batch: Dict):
    """vilt.py:455-459: what batch_collate yields -> the arguments of ViltContinualLearner.forward / process_inputs."""
    return {"images": batch["images"], "texts": batch["raw_texts"]}
