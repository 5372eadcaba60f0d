"""CPU: the criterion boundary of the HIP path -- which ``torch.nn`` criteria have a fused kernel kind, which are refused, and
what the trainer does with each (no GPU: only host logic and the C header)."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LBD = {"class": 1.0, "cycle": 5.0, "idt": 5.0, "reg": 0.5, "idt_reg": 0.5, "KL": 0.0, "batch_KL": 0.0, "corr_enc": 0.0, "hist": 0.0}


def _trainer(criterion):
    from srgan_amd import model
    from srgan_amd.trainer import SRGAN_training
    G = model.SingleGenerator(3, 4, 2, 2, 1, "instance", num_con=12)
    D = model.SingleDiscriminator_solo_multi(3, 4, 2, 4, "instance", 4)
    E = model.Encoder(3, 8, 4, 4, "instance", 4, "cpu")
    return SRGAN_training([G, D, E], [None, None, None], criterion, dict(LBD), 1, "cpu", np.eye(4), 4, "mu", 8)


@pytest.mark.parametrize("gan,cls", [(nn.BCEWithLogitsLoss, nn.BCELoss), (nn.BCEWithLogitsLoss, nn.MSELoss),
                                     (nn.MSELoss, nn.BCELoss)])
def test_bce_criteria_keep_the_fused_paths(gan, cls):
    sg = _trainer([gan(), cls()])
    assert sg._fused_paths()
    assert sg._class_is_mse() == (cls is nn.MSELoss)          # keeps its meaning: "criterion_class is nn.MSELoss()"
    from srgan_amd import ops
    assert sg._kinds() == (ops.CRIT_BCE if gan is nn.BCEWithLogitsLoss else ops.CRIT_MSE,
                           ops.CRIT_BCE if cls is nn.BCELoss else ops.CRIT_MSE)


def test_accepted_criteria_reach_the_kernels_and_have_no_cpu_fallback():
    from srgan_amd import losses
    from srgan_amd._lib import SrganHipError
    with pytest.raises(SrganHipError, match="no CPU fallback"):
        losses.get_loss_D([torch.zeros(2, 1, 3, 3)], 1.0, nn.BCEWithLogitsLoss())
    with pytest.raises(SrganHipError, match="no CPU fallback"):
        losses.get_domainloss_D([torch.full((2, 4), 0.25)], torch.eye(4)[:2], nn.BCELoss())


REFUSED_GAN = [lambda: nn.BCEWithLogitsLoss(pos_weight=torch.ones(1)), lambda: nn.BCEWithLogitsLoss(weight=torch.ones(1)),
               lambda: nn.BCEWithLogitsLoss(reduction="sum"), lambda: nn.BCEWithLogitsLoss(reduction="none"),
               lambda: nn.BCELoss(), lambda: nn.L1Loss(), lambda: nn.MSELoss(reduction="sum"), lambda: nn.HingeEmbeddingLoss()]
REFUSED_CLASS = [lambda: nn.BCELoss(weight=torch.ones(4)), lambda: nn.BCELoss(reduction="sum"), lambda: nn.BCEWithLogitsLoss(),
                 lambda: nn.L1Loss(), lambda: nn.MSELoss(reduction="sum"), lambda: nn.CrossEntropyLoss()]


@pytest.mark.parametrize("make", REFUSED_GAN)
def test_refused_gan_criteria(make):
    from srgan_amd import losses
    with pytest.raises(NotImplementedError, match="nn.MSELoss"):
        losses.get_loss_D([torch.zeros(2, 1, 3, 3)], 1.0, make())
    assert not _trainer([make(), nn.MSELoss()])._fused_paths()


@pytest.mark.parametrize("make", REFUSED_CLASS)
def test_refused_class_criteria(make):
    from srgan_amd import losses
    with pytest.raises(NotImplementedError, match="nn.MSELoss"):
        losses.get_domainloss_D([torch.full((2, 4), 0.25)], torch.eye(4)[:2], make())
    sg = _trainer([nn.MSELoss(), make()])
    assert not sg._fused_paths() and not sg._class_is_mse()


def test_unsupported_gan_criterion_is_not_replaced_by_lsgan():
    """``update_D`` and the generator's ``D(target_image)`` term used to look at ``criterion_class`` only: a trainer built with
    ``[nn.L1Loss(), nn.MSELoss()]`` took the fused one-launch path and silently trained LSGAN.  It must leave the fused paths
    (the generic path then asks ``get_loss_D``, which raises)."""
    sg = _trainer([nn.L1Loss(), nn.MSELoss()])
    assert sg._class_is_mse() and not sg._fused_paths()
    with pytest.raises(NotImplementedError, match="nn.MSELoss"):
        sg._kinds()
    with pytest.raises(NotImplementedError, match="enable_graph"):
        sg.opt_sche_initialization()
        sg.enable_graph()


def test_header_declares_the_criterion_kinds_and_entry_points():
    header = open(os.path.join(ROOT, "include", "srgan_hip.h")).read()
    assert re.search(r"enum\s*\{\s*SRGAN_CRIT_MSE\s*=\s*0\s*,\s*SRGAN_CRIT_BCE\s*=\s*1\s*\}", header)
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    from srgan_amd import _lib, ops
    assert (ops.CRIT_MSE, ops.CRIT_BCE) == (0, 1)
    for name, n_args in (("srgan_crit_const", 8), ("srgan_softmax_crit", 10), ("srgan_crit_pair", 9), ("srgan_d_losses_crit", 17)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", code)
        assert m, name
        assert len(m.group(1).split(",")) == n_args and "kind" in m.group(1), name
        assert len(_lib.SIGNATURES[name][1]) == n_args, name
    # every entry point cites its reference call site
    for name in ("srgan_crit_const", "srgan_softmax_crit", "srgan_crit_pair", "srgan_d_losses_crit"):
        before = header[:header.index("int " + name + "(")]
        assert "util.py:4" in before[before.rindex("/*"):], name
