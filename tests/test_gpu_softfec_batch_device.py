"""k_soft_fec_batch by itself on the MI355X: tests/gpu/softfec_batch_device_driver.hip links beside the shipped
gr_adsb_amd/csrc/adsb_softfec_batch.hip and runs its launcher on guarded device buffers, every item's samples in an allocation
of its own.  Every kernel case of tests/test_softfec_batch.py runs unchanged (the driver has the emulator driver's entry point),
so the device's bytes equal the restatement's, item by item."""
import ctypes

import pytest

import device_build
import test_softfec_batch as TB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sim():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    so = device_build.device_lib("adsb_softfec_batch.hip", "softfec_batch_device_driver.hip", "libadsb_softfec_batch_device.so",
                                 ["adsb_softfec_batch.h", "adsb_softfec_batch_device.h", "adsb_softfec_device.h", "adsb_reply_device.h",
                                  "adsb_env_hip.h"])
    return ctypes.CDLL(so)


@pytest.mark.parametrize("rule", sorted(TB.RULES))
def test_items_of_0_1_4_5_9_records_at_their_own_origins(sim, rule):
    TB.test_items_of_0_1_4_5_9_records_at_their_own_origins(sim, rule)


def test_an_empty_item_and_a_fallback_item_between_full_ones(sim):
    TB.test_an_empty_item_and_a_fallback_item_between_full_ones(sim)


def test_the_same_record_in_two_neighbouring_items_reads_its_own_samples(sim):
    TB.test_the_same_record_in_two_neighbouring_items_reads_its_own_samples(sim)


def test_a_mirror_shorter_than_the_list(sim):
    TB.test_a_mirror_shorter_than_the_list(sim)


def test_ten_samples_per_microsecond(sim):
    TB.test_ten_samples_per_microsecond(sim)


@pytest.mark.parametrize("k", range(5))
def test_every_input_format(sim, k):
    TB.test_every_input_format(sim, k)
