"""Block sparsity for the loop layers of WaveRNN (Kalchbrenner et al. 2018, "Efficient Neural Audio Synthesis", section 3): the blocks,
magnitude pruning in those blocks, and the schedule that prunes while training.

A block is what ``kernel='teamg'`` / ``'teamg_batch'`` can leave out with ``teamg_sparse = True``: 64 consecutive
elements of one padded row of the kernels' weight image, i.e. of one output row of one matrix --

* ``fc3.weight``, ``fc2.weight``, ``fc1.weight``: 64-column chunks from column 0;
* ``rnn*.weight_ih_l0`` and, separately, ``rnn*.weight_hh_l0``: 64-column chunks of every gate row;
* ``I.weight[:, 1:]``: 64-column chunks from column 1 (column 0, the fed-back sample, stays a dense vector).

The last chunk of a row is short where the row length is no multiple of 64.  Nothing here needs a device.
"""
import math
from collections import namedtuple
from typing import Dict, Iterable, Optional

import torch

BLOCK = 64
LAYERS = ('fc3', 'fc2', 'fc1', 'rnn2', 'rnn1', 'cond')       # _cabi.TEAMG_LAYER_NAMES
PRUNED_BY_DEFAULT = ('rnn1', 'rnn2', 'fc1', 'fc2')

# one operand segment of a layer's rows: columns [col0, col0 + cols) of state-dict tensor `tensor`, `blocks` = ceil(cols / 64) per row
Segment = namedtuple('Segment', 'tensor col0 cols blocks')


def _segment(tensor: str, col0: int, cols: int) -> Segment:
    return Segment(tensor, col0, cols, (cols + BLOCK - 1) // BLOCK)


def _layout(H: int, FC: int, F: int, A: int, NC: int) -> dict:
    def layer(rows, *segs):
        return dict(rows=rows, segments=list(segs), blocks=sum(s.blocks for s in segs))
    return {
        'fc3': layer(NC, _segment('fc3.weight', 0, FC)),
        'fc2': layer(FC, _segment('fc2.weight', 0, FC + A)),
        'fc1': layer(FC, _segment('fc1.weight', 0, H + A)),
        'rnn2': layer(3 * H, _segment('rnn2.weight_ih_l0', 0, H + A), _segment('rnn2.weight_hh_l0', 0, H)),
        'rnn1': layer(3 * H, _segment('rnn1.weight_ih_l0', 0, H), _segment('rnn1.weight_hh_l0', 0, H)),
        'cond': layer(H, _segment('I.weight', 1, F + A)),
    }


def block_layout(dims: dict, mode: str = 'RAW') -> dict:
    """The blocks of the six loop layers in model coordinates.  ``dims``: the constructor dims (``rnn_dims``, ``fc_dims``, ``bits``,
    ``feat_dims``, ``res_out_dims``; other keys are ignored).  Returns layer name -> ``dict(rows, segments, blocks)``: ``rows`` output
    rows (gate rows for a GRU layer), ``segments`` a list of :class:`Segment` (one per matrix of the row), ``blocks`` the blocks of one
    row -- ``k_padded / 64`` of ``_cabi.teamg_plan``."""
    if mode not in ('RAW', 'MOL'):
        raise ValueError(f"mode must be 'RAW' or 'MOL', not {mode!r}")
    return _layout(int(dims['rnn_dims']), int(dims['fc_dims']), int(dims['feat_dims']), int(dims['res_out_dims']) // 4,
                   2 ** int(dims['bits']) if mode == 'RAW' else 30)


def _state(model_or_state_dict) -> dict:
    sd = model_or_state_dict.state_dict() if hasattr(model_or_state_dict, 'state_dict') else model_or_state_dict
    return {k: (v if isinstance(v, torch.Tensor) else torch.as_tensor(v)) for k, v in sd.items()}


def _layout_of_state(sd: dict) -> dict:
    H, FC = sd['rnn1.weight_hh_l0'].shape[1], sd['fc3.weight'].shape[1]
    A = sd['fc2.weight'].shape[1] - FC
    return _layout(H, FC, sd['I.weight'].shape[1] - 1 - A, A, sd['fc3.weight'].shape[0])


def block_norms(w: torch.Tensor) -> torch.Tensor:
    """Squared L2 norm (float64) of every 64-column block of the rows of ``w`` (rows, cols) -> (rows, ceil(cols / 64))."""
    rows, cols = w.shape
    nb = (cols + BLOCK - 1) // BLOCK
    wp = torch.nn.functional.pad(w.detach().double(), (0, nb * BLOCK - cols))
    return (wp.view(rows, nb, BLOCK) ** 2).sum(-1)


def kept_blocks(density: float, blocks: int) -> int:
    """Blocks a row of ``blocks`` blocks keeps at ``density``: ``ceil(density * blocks)``."""
    return min(blocks, int(math.ceil(density * blocks - 1e-9)))


def block_masks(model_or_state_dict, density: float, layers: Iterable[str] = PRUNED_BY_DEFAULT, keep: Optional[Dict[str, torch.Tensor]] = None
                ) -> Dict[str, torch.Tensor]:
    """Row-balanced magnitude pruning in blocks.  Per output row and segment of every layer in ``layers`` the ``ceil(density * blocks)``
    blocks of largest L2 norm stay, ties going to the lower index; the rest of the row is to be zeroed.  Returns state-dict key -> bool
    tensor of the parameter's shape (``True``: the weight stays); column 0 of ``I.weight`` is always ``True``.  Biases, the upsample
    network and layers not named get no mask.  ``density=1`` keeps everything; outside (0, 1] is a ``ValueError``.  ``keep``: earlier
    masks; the result is their intersection with the new ones (a pruned block stays pruned).  Apply with :func:`apply_masks_`."""
    if isinstance(density, bool) or not isinstance(density, (int, float)) or not 0.0 < float(density) <= 1.0:
        raise ValueError(f'density must be in (0, 1], not {density!r}')
    layers = tuple(layers)
    for name in layers:
        if name not in LAYERS:
            raise ValueError(f'layers: {name!r} is none of {LAYERS}')
    sd = _state(model_or_state_dict)
    layout = _layout_of_state(sd)
    masks = {}
    for name in layers:
        for seg in layout[name]['segments']:
            w = sd[seg.tensor]
            part = w[:, seg.col0:seg.col0 + seg.cols]
            order = torch.argsort(-block_norms(part), dim=1, stable=True)
            kb = torch.zeros(part.shape[0], seg.blocks, dtype=torch.bool, device=w.device)
            kb.scatter_(1, order[:, :kept_blocks(float(density), seg.blocks)], True)
            m = torch.ones(w.shape, dtype=torch.bool, device=w.device)
            m[:, seg.col0:seg.col0 + seg.cols] = kb.repeat_interleave(BLOCK, dim=1)[:, :seg.cols]
            if keep is not None and seg.tensor in keep:
                m &= keep[seg.tensor].to(m.device)
            masks[seg.tensor] = m
    return masks


def apply_masks_(model, masks: Dict[str, torch.Tensor]):
    """Zero, in place, every weight of ``model`` whose mask is ``False`` (exactly zero, whatever it held).  Returns ``model``."""
    params = dict(model.named_parameters())
    with torch.no_grad():
        for key, m in masks.items():
            params[key].masked_fill_(~m.to(params[key].device), 0.0)
    return model


class SparsitySchedule:
    """The paper's pruning schedule: the pruned share of every row rises from 0 at step ``start`` to ``1 - target_density`` at step ``end``
    as ``(1 - target_density) (1 - (1 - (t - start) / (end - start))^3)``, re-evaluated every ``every`` steps (and at ``end``).  Before
    ``start`` nothing is pruned, after ``end`` the masks stay.  ``layers``: what :func:`block_masks` prunes."""

    def __init__(self, target_density: float, start: int, end: int, every: int = 1, layers: Iterable[str] = PRUNED_BY_DEFAULT):
        if isinstance(target_density, bool) or not isinstance(target_density, (int, float)) or not 0.0 < float(target_density) <= 1.0:
            raise ValueError(f'target_density must be in (0, 1], not {target_density!r}')
        if int(start) < 0 or int(end) < int(start) or int(every) < 1:
            raise ValueError(f'SparsitySchedule: need 0 <= start <= end and every >= 1, not start={start}, end={end}, every={every}')
        self.target_density, self.start, self.end, self.every, self.layers = float(target_density), int(start), int(end), int(every), tuple(layers)

    def pruned_share(self, step: int) -> float:
        if step < self.start:
            return 0.0
        if step >= self.end:
            return 1.0 - self.target_density
        return (1.0 - self.target_density) * (1.0 - (1.0 - (step - self.start) / (self.end - self.start)) ** 3)

    def density(self, step: int) -> float:
        return 1.0 - self.pruned_share(step)

    def due(self, step: int) -> bool:
        """Whether the masks are recomputed at ``step``."""
        return self.start <= step <= self.end and ((step - self.start) % self.every == 0 or step == self.end)
