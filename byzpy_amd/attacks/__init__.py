from byzpy_amd.attacks.base import Attack
from byzpy_amd.attacks.ops import (
    AGRTailoredAttack,
    CoordinateTailoredAttack,
    EmpireAttack,
    GaussianAttack,
    InfAttack,
    LabelFlipAttack,
    LittleAttack,
    MimicAttack,
    MinMaxAttack,
    MinSumAttack,
    SignFlipAttack,
)

__all__ = [
    "Attack",
    "EmpireAttack",
    "SignFlipAttack",
    "LabelFlipAttack",
    "LittleAttack",
    "GaussianAttack",
    "InfAttack",
    "MimicAttack",
    "MinMaxAttack",
    "MinSumAttack",
    "AGRTailoredAttack",
    "CoordinateTailoredAttack",
]
