"""MoCo v3 baseline (reference other_baselines/mocov3): the model, LARS and their HIP launches."""
