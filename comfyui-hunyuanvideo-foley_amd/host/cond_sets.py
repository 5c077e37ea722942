"""Per-clip conditioning: the distinct conditioning sets of a batch and the maps from batch rows to them (pure CPU logic).

A batch row is (cfg half h, clip k), row b = h*clips + k, in the [uncond ; cond] order of utils.py:193-195 - or, with separate
video and text guidance (`three`), the three halves [negative prompt + empty rows ; negative prompt + video ; prompt + video].  Every row reads one
text set (its prompt, or its negative prompt in the unconditional half) and one visual set (its SigLIP2 and Synchformer features
together; the learned empty rows in the unconditional half).  Sets are de-duplicated within each cfg half by exact equality of
their fp32 rows, so a batch whose clips share their conditioning has exactly one set per half - the plan foley_prepare takes
unchanged - and a video batch of 6 clips under CFG has 1 + 6 visual sets, not 12.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch


class CondSetsError(ValueError):
    pass


# A batch whose clips differ in their visual features lays the sync rows out per batch row; the library's periodicity check of
# those rows serves at most 32 of them (foley_prepare_sets).  Prompts alone have no such cap.
# 16 clips under CFG, 10 with three guidance halves.
MAX_VISUAL_ROWS = 32


@dataclass
class CondSets:
    text: torch.Tensor                  # [n_text, Lt, cond_dim]
    clip: torch.Tensor                  # [n_vis, Lv, clip_dim]
    sync: torch.Tensor                  # [n_vis, Ls, sync_dim]
    text_of: Optional[List[int]]        # [ncfg*clips] batch row -> text set; None: one set per cfg half (foley_prepare)
    vis_of: Optional[List[int]]         # [ncfg*clips] batch row -> visual set; None together with text_of

    @property
    def homogeneous(self) -> bool:
        return self.text_of is None


def batch_of(t: torch.Tensor, batch_size: int, what: str) -> int:
    """Batch of one conditioning tensor: 1 (shared by every clip) or batch_size (one row per clip)."""
    if t.dim() != 3:
        raise CondSetsError(f"{what} must be [batch, tokens, channels], got {tuple(t.shape)}")
    if t.shape[0] not in (1, batch_size):
        raise CondSetsError(f"{what} has batch {t.shape[0]}: conditioning tensors have batch 1 (shared by all clips) or "
                            f"batch_size ({batch_size}, one row per clip)")
    return t.shape[0]


def dedup(rows: Sequence[torch.Tensor]) -> Tuple[List[torch.Tensor], List[int]]:
    """Distinct rows (exact torch.equal) in order of first appearance, and the index of every row's set."""
    sets: List[torch.Tensor] = []
    idx: List[int] = []
    for r in rows:
        for j, s in enumerate(sets):
            if s.shape == r.shape and torch.equal(s, r):
                idx.append(j)
                break
        else:
            idx.append(len(sets))
            sets.append(r)
    return sets, idx


def build(text: torch.Tensor, unc: torch.Tensor, clip: torch.Tensor, sync: torch.Tensor, empty_clip: torch.Tensor,
          empty_sync: torch.Tensor, batch_size: int, cfg: bool, three: bool = False) -> CondSets:
    """text / unc [1 or batch_size, Lt, C] (padded to one Lt), clip [1 or bs, Lv, C], sync [1 or bs, Ls, C], all fp32;
    empty_clip / empty_sync: the learned rows [C] that stand for the visual features in the unconditional half under CFG.
    three: the halves of separate video and text guidance - the unconditional half, then the negative prompt with the clip's
    visual features, then the conditional half; sets are still de-duplicated per half."""
    if three and not cfg:
        raise CondSetsError("three halves are a form of classifier-free guidance: cfg must be set")
    for t, n in ((text, "text_feat"), (unc, "uncond_text_feat"), (clip, "siglip2_feat"), (sync, "syncformer_feat")):
        batch_of(t, batch_size, n)
    if text.shape[1:] != unc.shape[1:]:
        raise CondSetsError("text_feat and uncond_text_feat must be padded to one length")
    row = lambda t, k: t[k if t.shape[0] > 1 else 0]
    halves_t = ([[row(unc, k) for k in range(batch_size)]] * (2 if three else 1) if cfg else []) + [[row(text, k) for k in range(batch_size)]]
    Lv, Ls = clip.shape[1], sync.shape[1]
    e_clip = empty_clip.reshape(1, -1).to(clip).expand(Lv, -1)
    e_sync = empty_sync.reshape(1, -1).to(sync).expand(Ls, -1)
    halves_v = ([[(e_clip, e_sync)] * batch_size] if cfg else []) + [[(row(clip, k), row(sync, k)) for k in range(batch_size)]] * (2 if three else 1)
    t_sets: List[torch.Tensor] = []
    v_sets: List[Tuple[torch.Tensor, torch.Tensor]] = []
    text_of: List[int] = []
    vis_of: List[int] = []
    for ht, hv in zip(halves_t, halves_v):
        s, i = dedup(ht)
        text_of += [len(t_sets) + j for j in i]
        t_sets += s
        s, i = dedup([torch.cat([c.flatten(), y.flatten()]) for c, y in hv])     # clip and sync rows are one visual set
        vis_of += [len(v_sets) + j for j in i]
        v_sets += [hv[i.index(j)] for j in range(len(s))]
    ncfg = len(halves_t)
    per_half = [b // batch_size for b in range(ncfg * batch_size)]
    out = CondSets(torch.stack(t_sets), torch.stack([c for c, _ in v_sets]), torch.stack([y for _, y in v_sets]),
                   text_of, vis_of)
    if text_of == per_half and vis_of == per_half:
        out.text_of = out.vis_of = None
    elif vis_of != per_half and len(vis_of) > MAX_VISUAL_ROWS:
        raise CondSetsError(f"per-clip visual features take at most {MAX_VISUAL_ROWS} batch rows ({MAX_VISUAL_ROWS // ncfg} clips"
                            f"{' with three guidance halves' if three else ' under CFG' if cfg else ''}); this batch has {len(vis_of)}: split it into smaller batches")
    return out


def stack_features(parts: Sequence[Dict[str, torch.Tensor]], keys: Sequence[str]) -> Dict[str, torch.Tensor]:
    """One feature dict per clip (batch 1 each) -> one dict of batch len(parts); refuses clips of different token counts."""
    out = {}
    for k in keys:
        ts = [p[k].reshape(-1, *p[k].shape[-2:]) for p in parts]
        if len({tuple(t.shape) for t in ts}) != 1:
            raise CondSetsError(f"{k}: the clips have different shapes {[tuple(t.shape) for t in ts]} - the clips of a batch "
                                "share one duration")
        out[k] = torch.cat(ts)
    return out


def shard(feats: Dict[str, torch.Tensor], lo: int, hi: int, batch_size: int) -> Dict[str, torch.Tensor]:
    """The clips [lo, hi) of a feature dict: per-clip tensors (batch batch_size > 1) are sliced, shared ones (batch 1) kept."""
    return {k: (v[lo:hi] if torch.is_tensor(v) and v.dim() == 3 and batch_size > 1 and v.shape[0] == batch_size else v)
            for k, v in feats.items()}
