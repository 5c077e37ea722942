"""LoRA adapters for a HUNYUAN_MODEL: parse the adapter files in circulation, then merge them into the packed weights.

    lora.ensure(model, [("foley_style.safetensors", 0.8), (state_dict, -0.3)])     # merge exactly this set
    lora.ensure(model, None)                                                      # back to the loaded weights, bit for bit

The arithmetic lives in the library (csrc/lora.hip, foley_lora_*): for a checkpoint tensor W[O, I(, k)] and the adapters of the
list in order,  stored' = rnd_store(f32(pristine) + sum_j s_j * up_j @ down_j)  with  s_j = fl32(strength_j * alpha_j / r_j)  (no
alpha: fl32(strength_j)) formed in fp64 here, always from the pristine values with one rounding.  The merge is in place at
unchanged addresses: the captured loop stays valid and runs at the plain speed, and an fp8 arena stays fp8.

Formats served (module = a reference module path such as `single_blocks.7.linear2.w1`):
  * PEFT / diffusers   [base_model.model.|diffusion_model.|transformer.|model.]<module>.lora_A.weight / .lora_B.weight
  * ComfyUI-native     <module>.lora_down.weight / .lora_up.weight / .alpha
  * kohya              lora_unet_<module with dots as underscores>.lora_down.weight / .lora_up.weight / .alpha - module names
                       contain underscores themselves, so the spelling is resolved through a table built from the model's own
                       module list, not by splitting
Refused by name, before anything touches the device: DoRA (`dora_scale`), LoKr (`lokr_*`), LoHa (`hada_*`), `lora_mid`, full
and bias diffs (`.diff`, `.diff_b`), a key that resolves to no module, a module with only one half of its pair.
"""
from __future__ import annotations

import logging
import os
import struct
from collections import OrderedDict
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import synth
from .config import XXL, DiTConfig

log = logging.getLogger("foley_amd.lora")

PREFIXES = ("base_model.model.", "diffusion_model.", "transformer.", "model.")
KOHYA_PREFIX = "lora_unet_"
_DOWN, _UP, _ALPHA = "down", "up", "alpha"
_SUFFIXES = ((".lora_A.weight", _DOWN), (".lora_B.weight", _UP), (".lora_down.weight", _DOWN), (".lora_up.weight", _UP),
             (".alpha", _ALPHA))
_UNSUPPORTED = (("dora_scale", "DoRA (dora_scale) is not supported"), ("lokr_", "LoKr (lokr_*) is not supported"),
                ("hada_", "LoHa (hada_*) is not supported"), ("lora_mid", "a lora_mid (Tucker / conv-mid) factor is not supported"))
OPERAND_DTYPES = (torch.float32, torch.bfloat16, torch.float16)
MAX_RANK, MAX_ADAPTERS = 256, 8


class LoraError(ValueError):
    """An adapter this package does not serve; the message names the key and the reason."""


def modules(cfg: DiTConfig) -> List[str]:
    """Reference module paths whose `.weight` is a matrix of the DiT (what an adapter may target), from the model's own schema."""
    return [k[:-len(".weight")] for k, (shape, _s, _m) in synth.dit_schema(cfg).items() if k.endswith(".weight") and len(shape) >= 2]


def kohya_table(cfg: DiTConfig) -> Dict[str, str]:
    """`single_blocks_1_linear2_w1` -> `single_blocks.1.linear2.w1` for every module of the model."""
    return {m.replace(".", "_"): m for m in modules(cfg)}


def _resolve(name: str, mods, kohya) -> Optional[str]:
    if name.startswith(KOHYA_PREFIX):
        return kohya.get(name[len(KOHYA_PREFIX):])
    stripped = True
    while stripped and name not in mods:       # prefixes stack (`base_model.model.diffusion_model.`)
        stripped = False
        for p in PREFIXES:
            if name.startswith(p):
                name, stripped = name[len(p):], True
                break
    return name if name in mods else None


def load(src, cfg: DiTConfig = XXL) -> "OrderedDict[str, Tuple[torch.Tensor, torch.Tensor, Optional[float]]]":
    """Adapter file (safetensors, or a tensors-only torch file) or state dict -> {reference key: (down, up, alpha or None)}, in
    the file's order.  Raises LoraError for everything the module docstring lists as refused."""
    if isinstance(src, (str, os.PathLike)):
        from .. import nodes
        sd = nodes._load_state_dict(src)
    else:
        sd = src
    mods = set(modules(cfg))
    kohya = kohya_table(cfg)
    parts: "OrderedDict[str, dict]" = OrderedDict()
    for k, v in sd.items():
        for marker, why in _UNSUPPORTED:
            if marker in k:
                raise LoraError(f"lora: '{k}': {why}")
        if k.endswith(".diff") or k.endswith(".diff_b"):
            raise LoraError(f"lora: '{k}': full-weight and bias diffs (.diff / .diff_b) are not supported")
        for suffix, role in _SUFFIXES:
            if k.endswith(suffix):
                name = k[:-len(suffix)]
                break
        else:
            raise LoraError(f"lora: '{k}': not an adapter tensor (expected .lora_A/.lora_B, .lora_down/.lora_up or .alpha)")
        module = _resolve(name, mods, kohya)
        if module is None:
            raise LoraError(f"lora: '{k}': resolves to no module of the {cfg.name} model")
        slot = parts.setdefault(module + ".weight", {})
        if role in slot:
            raise LoraError(f"lora: '{k}': a second {role} tensor for {module}")
        slot[role] = v
    out = OrderedDict()
    for key, p in parts.items():
        if _DOWN not in p or _UP not in p:
            have = _DOWN if _DOWN in p else _UP if _UP in p else _ALPHA
            raise LoraError(f"lora: '{key}': only one half of the pair (has {have} only)")
        alpha = p.get(_ALPHA)
        out[key] = (p[_DOWN], p[_UP], None if alpha is None else float(alpha))
    return out


def fl32(x: float) -> float:
    """Nearest fp32 of a Python float (fp64), as a Python float."""
    return struct.unpack("f", struct.pack("f", float(x)))[0]


def scale_of(strength: float, alpha: Optional[float], rank: int) -> float:
    """s = fl32(strength * alpha / rank), formed in fp64; without an alpha s = fl32(strength)."""
    return fl32(float(strength)) if alpha is None else fl32(float(strength) * float(alpha) / int(rank))


def _fingerprint(specs) -> tuple:
    fp = []
    for src, strength in specs:
        if isinstance(src, (str, os.PathLike)):
            st = os.stat(src)
            fp.append(("file", os.path.abspath(os.fspath(src)), st.st_size, st.st_mtime_ns, float(strength)))
        else:
            fp.append(("dict", id(src), float(strength)))
    return tuple(fp)


def normalize(specs) -> list:
    """[(path or dict, strength), ...] with the strength-0 entries dropped (they add nothing); None -> []."""
    out = []
    for item in specs or []:
        if not (isinstance(item, (tuple, list)) and len(item) == 2):
            raise LoraError("loras entries are (file name or state dict, strength) pairs")
        src, strength = item
        strength = float(strength)
        if strength != strength or strength in (float("inf"), float("-inf")):
            raise LoraError(f"lora: strength {strength} is not finite")
        if strength != 0.0:
            out.append((src, strength))
    return out


def _numel(shape) -> int:
    n = 1
    for v in shape:
        n *= int(v)
    return n


def _trim(shape) -> tuple:
    """A shape without its trailing singleton dimensions (a Linear weight [O, I] and a k=1 conv weight [O, I, 1] are one thing)."""
    s = [int(v) for v in shape]
    while len(s) > 1 and s[-1] == 1:
        s.pop()
    return tuple(s)


def plan_merge(specs, cfg: DiTConfig) -> "OrderedDict[str, list]":
    """{reference key: [(down, up, scale), ...]} in list order, everything checked that needs no device."""
    per_key: "OrderedDict[str, list]" = OrderedDict()
    schema = synth.dit_schema(cfg)
    for src, strength in specs:
        for key, (down, up, alpha) in load(src, cfg).items():
            if down.dtype not in OPERAND_DTYPES or up.dtype != down.dtype:
                raise LoraError(f"lora: '{key}': operand dtype must be f32, bf16 or f16 (down {down.dtype}, up {up.dtype})")
            if down.dim() < 2 or up.dim() < 2:
                raise LoraError(f"lora: '{key}': shape does not match (down {tuple(down.shape)}, up {tuple(up.shape)})")
            rank = int(down.shape[0])
            if not 1 <= rank <= MAX_RANK:
                raise LoraError(f"lora: '{key}': rank must be in [1, {MAX_RANK}], got {rank}")
            if up.dim() > 2 and _numel(up.shape[2:]) > 1:
                raise LoraError(f"lora: '{key}': up has a kernel > 1 (shape {tuple(up.shape)})")
            w = tuple(schema[key][0])
            if _trim(down.shape) != _trim((rank,) + w[1:]) or _trim(up.shape) != _trim((w[0], rank)):
                raise LoraError(f"lora: '{key}': shape does not match: the weight is {list(w)}, down {list(down.shape)}, "
                                f"up {list(up.shape)}")
            per_key.setdefault(key, []).append((down, up, scale_of(strength, alpha, rank)))
            if len(per_key[key]) > MAX_ADAPTERS:
                raise LoraError(f"lora: '{key}': more than {MAX_ADAPTERS} adapters on one key")
    return per_key


def merged(model) -> bool:
    return getattr(model, "_lora_fp", None) is not None


def ensure(model, specs: Optional[Sequence]) -> bool:
    """Make `model`'s weights the loaded ones plus exactly the adapters of `specs` = [(path or state dict, strength), ...], in
    that order.  The request is fingerprinted (file path + size + mtime or dict identity, strength, order): the same request
    again does nothing.  None / [] restores the loaded weights if a set is merged.  Strength 0 drops an adapter, negative
    strengths are allowed.  Everything that can be refused without the device is refused before it is touched; a refusal of the
    library leaves the model on its loaded weights.  Returns True if the weights changed.

    The host-side caches of a model (`_tables_cache`, `_timeline_cache`, host/sampler.py::build_plan) hold schedule, solver, RoPE,
    position and prompt-timeline tables only - nothing derived from a weight - so they stay; the library's own weight-derived
    tables are rebuilt by the foley_prepare every run starts with (foley_lora_end marks the context unprepared)."""
    specs = normalize(specs)
    fp = _fingerprint(specs) if specs else None
    if fp == getattr(model, "_lora_fp", None):
        return False
    ctx = model.ctx
    if not specs:
        ctx.lora_clear()
        model._lora_fp, model._lora_specs = None, None
        log.info("lora: restored the loaded weights")
        return True
    per_key = plan_merge(specs, model.cfg)
    keep = []                                     # the operands are borrowed until lora_end returns
    try:
        ctx.lora_begin()
        for key, adapters in per_key.items():
            dev = [(d.detach().to(model.device).contiguous(), u.detach().to(model.device).contiguous(), s) for d, u, s in adapters]
            keep.append(dev)
            ctx.lora_merge(key, dev)
        ctx.lora_end()
    except Exception:
        model._lora_fp, model._lora_specs = None, None
        ctx.lora_clear()
        raise
    model._lora_fp, model._lora_specs = fp, list(specs)
    log.info("lora: merged %d adapter(s) into %d tensors (%.1f MB of pristine copies)", len(specs), len(per_key),
             ctx.lora_backup_bytes() / 1e6)
    return True
