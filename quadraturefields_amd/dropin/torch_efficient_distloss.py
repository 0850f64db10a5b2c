"""``from torch_efficient_distloss import eff_distloss, eff_distloss_native, flatten_eff_distloss``
(train_finetune.py:33, train_ngp_nerf_sg_occ.py:27)."""
from quadraturefields_amd.losses import eff_distloss, eff_distloss_native, flatten_eff_distloss  # noqa: F401
