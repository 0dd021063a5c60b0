"""The reference's ``other_baselines`` package: baselines that train the same encoder."""
