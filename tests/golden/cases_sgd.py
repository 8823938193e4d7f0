"""Hyper-parameters of the NET_OPTIM = 'sgd' trajectory (tests/golden/traj_sgd.npz): shared by the generator
(make_golden_sgd.py, which needs the reference tree) and by the replay in tests/test_sgd_gpu.py (which does not).
Model, batches and the four injected samples are cases.traj_setup()'s.

  net_momentum / net_weight_decay / alpha_weight_decay: NET_MOMENTUM and the scripts' commented-in NET_WEIGHT_DECAY and
    ALPHA_WEIGHT_DECAY values (search_vqa.py:125-126,156), so that both decays are exercised;
  net_lr 0.05 (ten times NET_LR_BASE) and max_epoch 5: with clip 1.0 a step moves the weights by lr at most, and the two
    schedule steps of the trajectory change the rate visibly (x 0.906, then x 0.724) instead of by 1e-3 as at MAX_EPOCH 50."""
SGD_HYPER = dict(net_lr=0.05, net_lr_min=0.0005, net_momentum=0.9, net_weight_decay=1e-4, max_epoch=5, clip=1.0,
                 alpha_lr=0.1, alpha_betas=(0.0, 0.999), alpha_weight_decay=1e-3)
# weight steps w1, w2, w3 and the closing forward take these entries of traj_setup()'s plans (plans[2] is the arch step's)
SGD_WEIGHT_PLANS = (0, 1, 3, 0)
