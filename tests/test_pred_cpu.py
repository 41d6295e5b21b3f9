"""CPU: the one input contract of the meters' predictions (lm_net_amd.metrics._prediction, a pure function) and the size checks of
hip.confusion / hip.confusion_labels, which come before any device pointer is taken."""
import pytest
import torch

METERS = ("ConfusionMeter", "ImageStatsMeter", "SurfaceDistanceMeter")


def _prediction(*a):
    from lm_net_amd.metrics import _prediction as f
    return f(*a)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("label_dtype", [torch.uint8, torch.int64])
def test_logits_come_back_contiguous_fp32(dtype, label_dtype):
    lg = torch.arange(2 * 3 * 4 * 5, dtype=torch.float32).reshape(2, 3, 4, 5).to(dtype)
    out = _prediction(lg, 3, "ConfusionMeter", label_dtype)
    assert out.dtype == torch.float32 and out.shape == lg.shape and out.is_contiguous() and torch.equal(out, lg.float())
    nc = lg.permute(0, 1, 3, 2)                                      # a non-contiguous view
    assert not nc.is_contiguous()
    out = _prediction(nc, 3, "ConfusionMeter", label_dtype)
    assert out.is_contiguous() and out.dtype == torch.float32 and torch.equal(out, nc.float())


@pytest.mark.parametrize("dtype", [torch.uint8, torch.bool, torch.int32, torch.int64])
@pytest.mark.parametrize("label_dtype", [torch.uint8, torch.int64])
def test_label_maps_come_back_contiguous_in_the_label_dtype(dtype, label_dtype):
    m = (torch.arange(2 * 4 * 5).reshape(2, 4, 5) % 2).to(dtype)
    out = _prediction(m, 2, "ImageStatsMeter", label_dtype)
    assert out.dtype == label_dtype and out.shape == m.shape and out.is_contiguous() and torch.equal(out.long(), m.long())
    nc = m.transpose(1, 2)
    assert not nc.is_contiguous()
    out = _prediction(nc, 2, "ImageStatsMeter", label_dtype)
    assert out.is_contiguous() and out.dtype == label_dtype and torch.equal(out.long(), nc.long())


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_stray_values(dtype):
    """uint8 labels: -1 and everything >= 255 become 255 ("no class" for every n_classes <= 64); int64 labels: unchanged."""
    m = torch.tensor([[[0, 1, -1, 255, 300, 254, -7, 70000]]], dtype=dtype)
    assert _prediction(m, 2, "ConfusionMeter", torch.uint8).tolist() == [[[0, 1, 255, 255, 255, 254, 255, 255]]]
    assert _prediction(m, 2, "SurfaceDistanceMeter", torch.int64).tolist() == m.tolist()
    u8 = torch.tensor([[[0, 1, 255, 64]]], dtype=torch.uint8)        # a uint8 map passes as it is
    assert torch.equal(_prediction(u8, 2, "ImageStatsMeter", torch.uint8), u8)
    assert _prediction(u8, 2, "SurfaceDistanceMeter", torch.int64).tolist() == [[[0, 1, 255, 64]]]


@pytest.mark.parametrize("what", METERS)
def test_channel_mismatch_raises_for_every_meter(what):
    label_dtype = torch.int64 if what == "SurfaceDistanceMeter" else torch.uint8
    with pytest.raises(ValueError, match="%s: logits with 9 channels, n_classes = 2" % what):
        _prediction(torch.zeros(1, 9, 4, 4), 2, what, label_dtype)
    assert _prediction(torch.zeros(1, 9, 4, 4), 9, what, label_dtype).shape == (1, 9, 4, 4)


@pytest.mark.parametrize("what", METERS)
def test_neither_logits_nor_a_label_map_raises(what):
    for bad in (torch.zeros(1, 4, 4), torch.zeros(1, 4, 4, dtype=torch.float16),        # 3-D floating point
                torch.zeros(4, 4, dtype=torch.int64), torch.zeros(1, 2, 4, 4, 4),          # 2-D, 5-D
                torch.zeros(1, 2, 4, 4, dtype=torch.int64)):                               # 4-D integers are not logits
        for label_dtype in (torch.uint8, torch.int64):
            with pytest.raises(ValueError, match="%s: pred must be logits .* INTEGER label map" % what):
                _prediction(bad, 2, what, label_dtype)


def test_wrapper_size_checks_come_before_any_pointer():
    """CPU tensors: a wrong size raises ValueError; the pointer helpers would raise RuntimeError ("device tensor required")."""
    from lm_net_amd import hip
    lg, y = torch.zeros(2, 9, 4, 4), torch.zeros(2, 4, 4, dtype=torch.int64)
    for counts in (torch.zeros(2, 2), torch.zeros(9, 8), torch.zeros(82)):
        with pytest.raises(ValueError, match="confusion"):
            hip.confusion(lg, y, counts)
    with pytest.raises(ValueError, match="confusion"):
        hip.confusion(lg, y[:1], torch.zeros(9, 9))                  # labels of another size
    p8 = torch.zeros(2, 4, 4, dtype=torch.uint8)
    for counts in (torch.zeros(9, 8), torch.zeros(3, 3, 3), torch.zeros(4)):
        with pytest.raises(ValueError, match="confusion_labels"):
            hip.confusion_labels(p8, y, counts)
    with pytest.raises(ValueError, match="confusion_labels"):
        hip.confusion_labels(p8, y[:1], torch.zeros(9, 9))
    # right sizes reach the pointer helpers, which refuse CPU tensors
    with pytest.raises(RuntimeError):
        hip.confusion(lg, y, torch.zeros(9, 9))
    with pytest.raises(RuntimeError):
        hip.confusion_labels(p8, y, torch.zeros(9, 9))
