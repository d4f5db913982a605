"""What the float decode stores, restated in numpy (include/grk_mi355x.h,
grkgpu_decompress_float): with v the int32 value the integer decode gives for
output channel ch,

    f = float32(v) * float32(scale[ch]) + float32(bias[ch])

the product and the sum each rounded on their own in float32 (numpy never
contracts them), then f as it is (float32) or rounded to nearest even to
float16 (numpy's astype) / bfloat16 (torch's .to).  The tests compare bit
patterns, so -0.0 / +0.0, subnormals and inf count."""
import numpy as np

FLOATS = ("float32", "float16", "bfloat16")
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def per_channel(v, c):
    a = np.asarray(v, dtype=np.float64).reshape(-1)
    return np.array([a[k if a.size > 1 else 0] for k in range(c)], dtype=np.float32)


def normalise(v, scale, bias, name, layout="chw"):
    """The expected output for the integer decode v ((c,h,w), or (h,w,c) with
    layout="hwc", or a list of planes): a numpy array, a torch CPU tensor for
    bfloat16, a list of those for a list."""
    if isinstance(v, list):
        s, b = per_channel(scale, len(v)), per_channel(bias, len(v))
        return [normalise(p[None], s[k:k + 1], b[k:k + 1], name)[0] for k, p in enumerate(v)]
    v = np.asarray(v)
    c = v.shape[0] if layout == "chw" else v.shape[-1]
    shape = (c, 1, 1) if layout == "chw" else (1, 1, c)
    s, b = per_channel(scale, c).reshape(shape), per_channel(bias, c).reshape(shape)
    with np.errstate(over="ignore"):
        f = v.astype(np.float32) * s + b
        assert f.dtype == np.float32
        if name == "float32":
            return f
        if name == "float16":
            return f.astype(np.float16)
    import torch
    return torch.from_numpy(np.ascontiguousarray(f)).to(torch.bfloat16)


def bits(x):
    """The bit patterns of a float32 / float16 numpy array or of a float32 /
    float16 / bfloat16 tensor (any device), as uint32 / uint16."""
    if isinstance(x, np.ndarray):
        return x.view(np.uint32 if x.dtype == np.float32 else np.uint16)
    import torch
    x = x.detach().cpu().contiguous()
    if x.dtype == torch.float32:
        return x.numpy().view(np.uint32)
    return x.view(torch.int16).numpy().view(np.uint16)


def same_bits(got, want):
    if isinstance(want, list):
        return isinstance(got, list) and len(got) == len(want) and all(same_bits(g, w) for g, w in zip(got, want))
    g, w = bits(got), bits(want)
    return g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)
