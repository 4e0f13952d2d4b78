"""The augmentation curriculum of tokenizer fine-tuning (the ``--augs`` / ``--augs_schedule`` options of finetune.py): which
``(class, parameters)`` entries ``wmar_amd.utils.utils.apply_random_augmentation`` draws from in each epoch."""
from __future__ import annotations

from .geometric import Rotate, UpperLeftCropWithPadBack
from .valuemetric import JPEG, Brightness, GaussianBlur, GaussianNoise

STAGES = ("warmup", "weak", "medium", "strong")

_SMALL_ANGLES = [-3, -2, -1, 1, 2, 3]
_CROPS = [0.5, 0.6, 0.7, 0.8, 0.9]
# transform -> its candidate parameters in the weak, medium and strong stage (the warm-up stage augments nothing)
_STRENGTHS = {
    JPEG: ([90, 80, 70], [80, 60, 40], [40, 30, 20]),
    GaussianBlur: ([1, 3], [3, 5], [5, 7, 9]),
    GaussianNoise: ([0.005, 0.01, 0.015, 0.02], [0.02, 0.04, 0.06], [0.06, 0.08, 0.1]),
    Brightness: ([1.0, 1.1, 1.2], [1.2, 1.3, 1.4], [1.4, 1.7, 2.0]),
    Rotate: ([-1, 1], _SMALL_ANGLES, _SMALL_ANGLES),
    UpperLeftCropWithPadBack: ([0.8, 0.9], _CROPS, _CROPS),
}
TABLES = {"warmup": []}
for _i, _stage in enumerate(STAGES[1:]):
    TABLES[_stage] = [(cls, list(levels[_i])) for cls, levels in _STRENGTHS.items()]


def finetune_schedule(augs: str, augs_schedule, nb_epochs: int) -> dict:
    """``{epoch: [(cls, params), ...]}`` for epochs 0 .. nb_epochs - 1.  `augs` is ``"none"`` (an empty list every epoch) or
    ``"all+geom"``: `augs_schedule` -- ``"a,b,c,d"`` or a sequence of integers -- counts the epochs spent in each of `STAGES` in
    turn (fewer than four counts leave the later stages out) and must add up to `nb_epochs`."""
    if augs == "none":
        return {epoch: [] for epoch in range(nb_epochs)}
    if augs != "all+geom":
        raise ValueError(f"unknown augmentation set {augs!r}: expected 'none' or 'all+geom'")
    counts = [int(c) for c in (augs_schedule.split(",") if isinstance(augs_schedule, str) else augs_schedule)]
    assert sum(counts) == nb_epochs, f"the schedule {counts} covers {sum(counts)} epochs, the run has {nb_epochs}"
    stage_of_epoch = [stage for stage, n in zip(STAGES, counts) for _ in range(n)]
    return {epoch: TABLES[stage] for epoch, stage in enumerate(stage_of_epoch)}
