"""The reference's stage registries (test/__init__.py:6-22): stage classes are looked up by the names the command line uses."""
from . import detector, estimator, extractor, matcher
from .detector import yoho_det
from .estimator import (R_pre_log, extractor_dr_index, extractor_localtrans, refiner, sc2, yohoc, yohoc_ransac, yohoo, yohoo_ransac)
from .extractor import yoho_des
from .matcher import NMS_sample, mutual, yoho_mat

name2extractor = dict(yoho_des=yoho_des)
name2detector = dict(yoho_det=yoho_det)
name2matcher = dict(matmul=mutual, yoho_mat=yoho_mat)


class _Registry(dict):
    """A reference registry with this project's additions: the keys -- what iteration, len() and `in` see -- are the reference's names, which
    the drop-in aliases mirror; a stage the reference does not have is resolved on lookup (registry[name])."""

    def __init__(self, reference, additions):
        super().__init__(reference)
        self.additions = dict(additions)

    def __missing__(self, name):
        return self.additions[name]


name2estimator = _Registry(dict(yohoc=yohoc, yohoo=yohoo), dict(sc2=sc2))
