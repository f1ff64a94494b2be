"""The TDS encoder restated from its definition (tal/asr/models.py:298-397) at any kernel size, in a chosen dtype, with
torch.nn.functional.conv1d on the CPU.  Shared by tests/test_tds_ksize_cpu.py and tests/test_gpu_tds_ksize.py.

Weights are the deterministic synthetic ones of tal_asrd_amd.synth, keyed like the reference's state_dict (optionally under a
prefix, as tests/golden/make_golden_tds_ksize.py records them)."""
import numpy as np
import torch
import torch.nn.functional as F

from tal_asrd_amd import synth


def synth_weights(module, prefix=""):
    """{key: float32 tensor} of `module`'s state_dict filled as make_golden.fill does (keys without the prefix)."""
    shapes = {prefix + k: tuple(v.shape) for k, v in module.state_dict().items()}
    sd = synth.fill_state_dict(shapes)
    return {k[len(prefix):]: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}


def load_synth(module, prefix=""):
    """Load those weights into one of our modules (as make_golden.fill loads them into the reference's)."""
    own = module.state_dict()
    for k, v in synth_weights(module, prefix).items():
        own[k] = v.clone()
    module.load_state_dict(own)
    return module.eval()


def resize_conv(x, w, b, groups, dtype):
    """Conv1d(stride 2, padding 0) on [B, C, T]."""
    return F.conv1d(x.to(dtype), w.to(dtype), b.to(dtype), stride=2, groups=groups)


def block(x, sd, prefix, groups, k, dtype):
    """TDSBlock.forward (models.py:321-331) on [B, C, T]: x + rw relu(conv(x)); x + rw fc(x)."""
    x = x.to(dtype)
    rw = sd[prefix + "resweight"].to(dtype)
    c = F.conv1d(x, sd[prefix + "conv.0.weight"].to(dtype), sd[prefix + "conv.0.bias"].to(dtype), padding=k // 2, groups=groups)
    x = x + rw * torch.relu(c)
    h = torch.relu(F.conv1d(x, sd[prefix + "fc.0.weight"].to(dtype), sd[prefix + "fc.0.bias"].to(dtype)))
    return x + rw * F.conv1d(h, sd[prefix + "fc.3.weight"].to(dtype), sd[prefix + "fc.3.bias"].to(dtype))


def tds(x, sd, groups, depths, k, dtype, prefix=""):
    """TDS.forward (models.py:394-397) on [B, C, T]."""
    x = x.to(dtype)
    for i, d in enumerate(depths):
        x = resize_conv(x, sd["%sblocks.%d.0.weight" % (prefix, i)], sd["%sblocks.%d.0.bias" % (prefix, i)], groups, dtype)
        for j in range(d):
            x = block(x, sd, "%sblocks.%d.1.%d." % (prefix, i, j), groups, k, dtype)
    return x


def gconv_s2_tm(x, w, b, groups, dtype):
    """The resize conv on time-major [B, T, C] (the kernels' layout)."""
    return resize_conv(x.transpose(1, 2), w, b, groups, dtype).transpose(1, 2)


def gconv_res_tm(x, w, b, alpha, groups, dtype):
    """x + alpha * relu(Conv1d(padding k // 2)(x)) on time-major [B, T, C]."""
    xc = x.transpose(1, 2).to(dtype)
    c = F.conv1d(xc, w.to(dtype), b.to(dtype), padding=w.shape[-1] // 2, groups=groups)
    return (xc + alpha * torch.relu(c)).transpose(1, 2)
