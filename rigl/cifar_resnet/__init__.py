"""rigl.cifar_resnet: the reference's CIFAR module path; ``data_helper`` is served by rigl_amd.data."""
