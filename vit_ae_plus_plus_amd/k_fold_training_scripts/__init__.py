"""The reference's ``k_fold_training_scripts`` package: the supervised 3-D ResNet baseline and the helpers its pre-training scripts import."""
