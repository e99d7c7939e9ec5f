"""Point-wise backbones in front of the group-feature path (roreg_amd/testset.py)."""
