"""Entry point kept from the reference (train.py:21-36 ``train_MI_models``).  ``python train.py --synthetic`` trains
the MI critic on synthetic embeddings on the ROCm device; the real-data path of the reference (MIMIC-CXR JPEGs, a
private BERT checkpoint) is not available offline."""
import argparse
import os

import torch

from multi_modal import train_mutual_information
from mutual_info_img_txt._hip import check_estimator


def construct_training_parameters(argv=None):
    """The flags of the reference parser (helpers.py:84-144) that the hot path reads, plus the synthetic-mode ones."""
    p = argparse.ArgumentParser()
    p.add_argument('--batch_size', default=64, type=int)                       # helpers.py:110
    p.add_argument('--mi_estimator', default='dv', type=str)                   # helpers.py:122-124
    p.add_argument('--init_lr', default=1e-4, type=float)                      # helpers.py:125
    p.add_argument('--num_train_epochs', default=1, type=int)
    p.add_argument('--save_directory', default='save_dir/mm_synthetic', type=str)
    p.add_argument('--synthetic', action='store_true')
    p.add_argument('--critic', default='concat_mlp', choices=['concat_mlp', 'bilinear', 'separable'])
    p.add_argument('--embed_dim_img', default=128, type=int)
    p.add_argument('--embed_dim_txt', default=128, type=int)
    p.add_argument('--steps_per_epoch', default=20, type=int)
    p.add_argument('--precision', default='f32', choices=['bf16', 'f32', 'bf16x3'])  # the reference is fp32; bf16 is the fast mode
    p.add_argument('--synthetic_encoders', action='store_true')
    p.add_argument('--img_size', default=256, type=int)                        # helpers.py:130
    p.add_argument('--output_channels', default=1, type=int)                   # helpers.py:131
    p.add_argument('--embed_proj_dim', default=None, type=int)
    p.add_argument('--no_graph', dest='graph', action='store_false')
    p.add_argument('--seed', default=0, type=int)
    # hard-negative InfoNCE: train the row-wise / symmetric loss on each query's top-K negatives (a loss, not an MI bound)
    p.add_argument('--hard_negatives', default=None, type=int)
    # memory-bank InfoNCE: the row-wise / symmetric loss against the batch and a queue of the last K samples' embeddings
    # (ceiling log(batch + K); not checkpointed: the queue refills after a resume)
    p.add_argument('--memory_bank', default=None, type=int)
    # study-positive InfoNCE: the row-wise / symmetric loss with every same-study pair as a positive (a loss, not an MI
    # bound)
    p.add_argument('--study_positives', action='store_true')
    # soft-target InfoNCE: the row-wise / symmetric loss with targets from the finding labels of a CheXpert / NegBio label
    # table (a CSV with a study_id column); temperature and weight of the soft targets are required with it (a loss, not
    # an MI bound)
    p.add_argument('--soft_targets', default=None, type=str, metavar='CSV')
    p.add_argument('--soft_tau', default=None, type=float)
    p.add_argument('--soft_mix', default=None, type=float)
    p.add_argument('--soft_uncertain_positive', action='store_true')
    return p.parse_args(argv)


def check_training_parameters(args):
    """Eager validation of the flags that the reference only trips over inside the training step."""
    check_estimator(args.mi_estimator, args.critic)
    if getattr(args, "hard_negatives", None) is not None:
        from mutual_info_img_txt._hip import NCE_ESTIMATORS
        from mutual_info_img_txt.hard_negatives import check_k
        if args.mi_estimator not in NCE_ESTIMATORS:
            raise ValueError(f"--hard_negatives needs --mi_estimator in {sorted(NCE_ESTIMATORS)} "
                             f"(got {args.mi_estimator!r})")
        check_k(args.hard_negatives)
    if getattr(args, "memory_bank", None) is not None:
        from mutual_info_img_txt._hip import NCE_ESTIMATORS
        from mutual_info_img_txt.memory_bank import check_capacity
        if args.mi_estimator not in NCE_ESTIMATORS:
            raise ValueError(f"--memory_bank needs --mi_estimator in {sorted(NCE_ESTIMATORS)} "
                             f"(got {args.mi_estimator!r})")
        if getattr(args, "hard_negatives", None) is not None:
            raise ValueError("--memory_bank and --hard_negatives cannot be combined")
        check_capacity(args.memory_bank)
    if getattr(args, "study_positives", False):
        from mutual_info_img_txt._hip import NCE_ESTIMATORS
        if args.mi_estimator not in NCE_ESTIMATORS:
            raise ValueError(f"--study_positives needs --mi_estimator in {sorted(NCE_ESTIMATORS)} "
                             f"(got {args.mi_estimator!r})")
        if getattr(args, "hard_negatives", None) is not None or getattr(args, "memory_bank", None) is not None:
            raise ValueError("--study_positives cannot be combined with --hard_negatives or --memory_bank")
    if getattr(args, "soft_targets", None) is not None:
        from mutual_info_img_txt._hip import NCE_ESTIMATORS
        from mutual_info_img_txt.soft_targets import check_tau_mix
        if args.mi_estimator not in NCE_ESTIMATORS:
            raise ValueError(f"--soft_targets needs --mi_estimator in {sorted(NCE_ESTIMATORS)} "
                             f"(got {args.mi_estimator!r})")
        if (getattr(args, "hard_negatives", None) is not None or getattr(args, "memory_bank", None) is not None or
                getattr(args, "study_positives", False)):
            raise ValueError("--soft_targets cannot be combined with --hard_negatives, --memory_bank or --study_positives")
        if args.soft_tau is None or args.soft_mix is None:
            raise ValueError("--soft_targets needs both --soft_tau and --soft_mix")
        args.soft_tau, args.soft_mix = check_tau_mix(args.soft_tau, args.soft_mix)
    elif (getattr(args, "soft_tau", None) is not None or getattr(args, "soft_mix", None) is not None or
          getattr(args, "soft_uncertain_positive", False)):
        raise ValueError("--soft_tau, --soft_mix and --soft_uncertain_positive need --soft_targets CSV")
    return args


def train_MI_models(argv=None):
    args = check_training_parameters(construct_training_parameters(argv))
    if not torch.cuda.is_available():
        raise RuntimeError("the MI critic path needs an MI355X (ROCm) device; there is no CPU fallback")
    device = torch.device('cuda')
    args.save_directory = os.path.join(args.save_directory, f'mm_{args.mi_estimator}_epoch{args.num_train_epochs}')
    train_mutual_information(args, device)
    losses = train_mutual_information.last_manager.training_loss
    for n, l in enumerate(losses):
        print(f'Epoch {n+1} finished! Epoch loss: {l:.5f}')
    return losses


if __name__ == '__main__':
    train_MI_models()
