"""Down-stream training on the pre-trained encoder (reference: post_training_utils/)."""
