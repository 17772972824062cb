"""Which state-dict tensors train, travel to the server and stay with the client, per optimizer_mode (src/train/main.py:
114-118,141-163,248-250 and the personal-parameter shuttle of main.py:440-450,473-497).

  mode       trainable                      communicated (FedAvg)     personal (kept per client)
  dat        adapter_0, adapter_1, heads    adapter_1                 heads, adapter_0, adapter_2
  adapter    adapter, heads                 every 'adapter' key       heads ('task')
"""
from __future__ import annotations

from typing import Dict, List, Sequence

from . import lib as L

MODES = ("dat", "adapter")


def mode_names(keys: Sequence[str], mode: str) -> Dict[str, List[str]]:
    """{"trainable", "communicated", "personal"}: the subsets of `keys` (state-dict order kept) for optimizer_mode `mode`."""
    if mode not in MODES:
        raise L.FeddatHipError(f"optimizer_mode must be one of {MODES}, got {mode!r}")
    keys = list(keys)
    if mode == "dat":
        return dict(trainable=[k for k in keys if "task" in k or "adapter_0" in k or "adapter_1" in k],
                    communicated=[k for k in keys if "adapter_1" in k],
                    personal=[k for k in keys if "task" in k or "adapter_0" in k or "adapter_2" in k])
    return dict(trainable=[k for k in keys if "adapter" in k or "task" in k],
                communicated=[k for k in keys if "adapter" in k],
                personal=[k for k in keys if "task" in k])
