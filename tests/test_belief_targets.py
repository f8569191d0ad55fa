"""The belief-target option without a device: the training keys ``belief_targets`` /
``posterior_budget`` (ms_amd.train.belief_target_params), the shipped posterior config, and
collect_rollout's argument check."""
from __future__ import annotations

import os

import pytest

from conftest import ROOT

TRAINING = os.path.join(ROOT, "configs", "training")


def test_belief_target_keys():
    from ms_amd.posterior import TRAIN_BUDGET
    from ms_amd.train import belief_target_params
    assert belief_target_params({}) == ("hard", TRAIN_BUDGET)
    assert belief_target_params(None) == ("hard", TRAIN_BUDGET)
    assert belief_target_params({"belief_targets": "posterior"}) == ("posterior", TRAIN_BUDGET)
    assert belief_target_params({"belief_targets": "hard", "posterior_budget": 4096}) == ("hard", 4096)
    assert belief_target_params({"belief_targets": "hard"}, "posterior") == ("posterior", TRAIN_BUDGET)
    assert belief_target_params({"belief_targets": "posterior"}, "hard")[0] == "hard"
    for bad in ("soft", "Posterior", "", 1, True):
        with pytest.raises(ValueError):
            belief_target_params({"belief_targets": bad})
    with pytest.raises(ValueError):
        belief_target_params({}, "exact")
    for bad in (0, -1, (1 << 30) + 1):
        with pytest.raises(ValueError):
            belief_target_params({"posterior_budget": bad})
    assert 1 <= TRAIN_BUDGET <= 1 << 30 and TRAIN_BUDGET & (TRAIN_BUDGET - 1) == 0


def test_shipped_configs():
    """The posterior config is the medium config plus the one key; every other shipped config
    trains on hard labels."""
    from ms_amd.posterior import TRAIN_BUDGET
    from ms_amd.train import belief_target_params, load_config
    base = load_config(os.path.join(TRAINING, "16x16x40_medium.yaml"))
    post = load_config(os.path.join(TRAINING, "16x16x40_medium_posterior.yaml"))
    assert belief_target_params(post[3]["training"]) == ("posterior", TRAIN_BUDGET)
    assert post[:3] == base[:3]
    t = dict(post[3]["training"])
    assert t.pop("belief_targets") == "posterior"
    assert t == base[3]["training"] and set(post[3]) == set(base[3])
    for name in sorted(os.listdir(TRAINING)):
        if name != "16x16x40_medium_posterior.yaml":
            extras = load_config(os.path.join(TRAINING, name))[3]
            assert belief_target_params(extras.get("training", {}))[0] == "hard", name


def test_cli_flag_choices():
    from ms_amd.train import main
    with pytest.raises(SystemExit):  # argparse refuses the value before anything is set up
        main(["--belief_targets", "soft"])


def test_collect_rollout_rejects_unknown_targets():
    """Before the env, the model or the device is touched (none is given)."""
    from ms_amd.rollout import BELIEF_TARGETS, collect_rollout
    assert BELIEF_TARGETS == ("hard", "posterior")
    for bad in ("soft", "", None, "HARD"):
        with pytest.raises(ValueError, match="belief_targets"):
            collect_rollout(None, None, 4, "cpu", belief_targets=bad)


def test_library_exports_the_labels_header_symbol():
    """include/msposterior_labels.h declares one entry point, an addition to ABI version 3; its
    arguments are checked before any device work."""
    import re

    from ms_amd import _lib as L
    lib = L.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "msposterior_labels.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(ms_[a-z0-9_]+)\s*\(", src))) == ["ms_posterior_labels"]
    assert hasattr(lib, "ms_posterior_labels") and len(L.SIGNATURES["ms_posterior_labels"]) == 7
    assert L.ABI_VERSION == 3 and lib.ms_abi_version() == 3
    assert lib.ms_posterior_labels(None, 1 << 11, None, None, None, None, None) == 1  # MS_EINVAL
    assert b"null handle" in lib.ms_last_error()


def test_buffer_source_is_optional():
    import torch
    from ms_amd.buffers import RolloutBuffer
    plain = RolloutBuffer(4, 3, (10, 5, 5), 25, torch.device("cpu"), with_mine_labels=True)
    assert plain.mine_source is None and "mine_source" not in plain.slot(0)
    buf = RolloutBuffer(4, 3, (10, 5, 5), 25, torch.device("cpu"), with_mine_labels=True, with_mine_source=True)
    assert buf.mine_source.shape == (12,) and buf.mine_source.dtype == torch.uint8
    assert buf.slot(2)["mine_source"].data_ptr() == buf.mine_source[8:].data_ptr()
