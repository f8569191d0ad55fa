"""Imitation warm start from the exact-posterior player (ms_amd/imitate.py):

    python pretrain_il.py --config configs/imitation/16x16x40_medium.yaml --out runs/il
    python train_rl.py --config configs/training/16x16x40_medium.yaml --init_ckpt runs/il/ckpt_final.pt

Alternates collect_expert (the posterior player's states and targets, on device) and bc_update
(the HIP behaviour-cloning loss); writes train_metrics.csv, ckpt_latest.pt and ckpt_final.pt in
the Trainer's checkpoint format. One GPU. ``--augment`` shows every row under a fresh random board
symmetry per epoch and ``--epochs`` sets the passes over each buffer (DESIGN.md §16;
configs/imitation/16x16x40_medium_sym.yaml). ``--beta_start`` / ``--beta_end`` / ``--beta_decay_iters``
schedule the teacher's share of the moves per round and ``--learner`` picks the learner's own move
(greedy or sampled): a round whose beta is below 1 is collected on policy by collect_dagger, the
learner's states labelled by the teacher (DESIGN.md §17;
configs/imitation/16x16x40_medium_dagger.yaml)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "minesweeper-ppo_amd"))

from ms_amd.imitate import main  # noqa: E402

if __name__ == "__main__":
    main()
