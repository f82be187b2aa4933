"""The weight-image cache of an encoder (cppf_amd.models.model._DeviceWeights) on the host device, where no HIP device is needed:
one image per precision, each rebuilt in place and only when it is asked for.  Shared by test_pair_bf16_cpu.py and
test_sprin_bf16_cpu.py."""
import torch

OTHER = {"fp32": "bf16", "bf16": "fp32"}


def check(enc, param, tensor_of=lambda cached: cached):
    """enc: an encoder in eval mode on the host; param: one of its Parameters that both images hold; tensor_of: the image tensor
    inside what _packed_weights() returns"""
    def image():
        return tensor_of(enc._packed_weights("cpu"))

    # the second call returns the identical object, and so does _current_image()
    first = {}
    for prec in ("fp32", "bf16"):
        got = enc.set_precision(prec)._packed_weights("cpu")
        assert enc._packed_weights("cpu") is got and enc._current_image() is got
        first[prec] = tensor_of(got)
    assert first["fp32"].dtype == torch.float32 and first["bf16"].dtype == torch.int32
    assert first["fp32"].data_ptr() != first["bf16"].data_ptr()
    # switching back and forth returns each precision's own buffer
    for prec in ("fp32", "bf16", "fp32", "bf16"):
        enc.set_precision(prec)
        assert image() is first[prec]

    for prec in ("fp32", "bf16"):
        mine, other = first[prec], first[OTHER[prec]]
        enc.set_precision(prec)
        before, other_before = image().clone(), other.clone()
        with torch.no_grad():
            param.add_(0.25)                                   # what an optimizer step does
        now = image()
        assert now.data_ptr() == mine.data_ptr() and not torch.equal(now, before)          # rebuilt in place
        assert torch.equal(other, other_before)                                            # the other image: not touched ...
        enc.set_precision(OTHER[prec])
        assert tensor_of(enc._current_image()).data_ptr() == other.data_ptr() and torch.equal(other, other_before)
        later = image()                                                                     # ... until it is asked for
        assert later.data_ptr() == other.data_ptr() and not torch.equal(later, other_before)

        # a write that bypasses the version counter is seen after invalidate(), which forces the rebuild
        enc.set_precision(prec)
        before = image().clone()
        param.data.add_(0.25)
        assert torch.equal(image(), before)
        enc.invalidate()
        now = image()
        assert now.data_ptr() == mine.data_ptr() and not torch.equal(now, before)
