"""TEST INFRASTRUCTURE: the training step with frozen units (the reference's set_trainable, train.py:62-113) restated in
torch autograd -- oracle/train_ref.py's network with, per frozen unit, what Keras does for a layer with
trainable = False in TF 2.x:
  * its BatchNorm runs in inference mode inside the training call: (z - moving_mean) / sqrt(moving_variance + 1e-3)
    * gamma + beta, the moving statistics untouched;
  * its variables are not trainable (requires_grad=False): no gradient, and none in the returned dict;
  * the gradient still flows through it to trainable layers in front of it.
Units are named as trainer.train_units() names them ("pfn", "rpn/block2/0", "rpn/deconv1", "rpn/conv_box", ...)."""
import numpy as np
import torch
import torch.nn.functional as Fn

from oracle import loss_ref, nn_ref

BN_EPS = 1e-3


def _unit(name):
    parts = name.split("/")
    if parts[0] == "pfn":
        return "pfn"
    return "/".join(parts[:3] if parts[1].startswith("block") else parts[:2])


def _bn(x, t, w, pre, frozen, dims, dtype):
    shape = [1] * x.dim()
    cdim = [d for d in range(x.dim()) if d not in dims][0]
    shape[cdim] = -1
    g, b = t[pre + "/gamma"].reshape(shape), t[pre + "/beta"].reshape(shape)
    if frozen:
        mm = torch.tensor(np.asarray(w[pre + "/moving_mean"], np.float32), dtype=dtype).reshape(shape)
        mv = torch.tensor(np.asarray(w[pre + "/moving_variance"], np.float32), dtype=dtype).reshape(shape)
        return (x - mm) / torch.sqrt(mv + BN_EPS) * g + b
    mean = x.mean(dim=dims, keepdim=True)
    var = x.var(dim=dims, unbiased=False, keepdim=True)
    return (x - mean) / torch.sqrt(var + BN_EPS) * g + b


def training_step(d, w, example, labels, reg_targets, anchors, frozen=(), dtype=torch.float32):
    """Returns (loss dict of floats, gradient dict of the TRAINABLE tensors)."""
    frozen = set(frozen)
    voxels, num_points, coors = example[0], example[1], example[2]
    B = int(example[6].shape[0])
    names = [k for k in w if not k.endswith(("moving_mean", "moving_variance"))]
    t = {k: torch.tensor(np.asarray(w[k], dtype=np.float32), dtype=dtype, requires_grad=_unit(k) not in frozen)
         for k in names}
    feats = torch.from_numpy(nn_ref.pfn_decorate_np(voxels, num_points, coors, d.voxel_size, d.pc_range,
                                                    d.with_distance)).to(dtype)
    y = _bn(feats @ t["pfn/dense/kernel"], t, w, "pfn/bn", "pfn" in frozen, (0, 1), dtype)
    f = torch.relu(y).amax(dim=1)
    idx = torch.from_numpy((coors[:, 0].astype(np.int64) * d.ny + coors[:, 2]) * d.nx + coors[:, 3])
    canvas = torch.zeros(B * d.ny * d.nx, f.shape[1], dtype=dtype).index_add(0, idx, f).reshape(B, d.ny, d.nx, -1)
    x = canvas.permute(0, 3, 1, 2)
    ups = []
    for b in range(3):
        for j in range(d.layer_nums[b] + 1):
            pre = f"rpn/block{b + 1}/{j}"
            stride = d.layer_strides[b] if j == 0 else 1
            x = Fn.conv2d(x, t[pre + "/depthwise_kernel"].permute(2, 3, 0, 1), stride=stride, padding=1, groups=x.shape[1])
            x = Fn.conv2d(x, t[pre + "/pointwise_kernel"].permute(3, 2, 0, 1))
            x = torch.relu(_bn(x, t, w, pre + "/bn", pre in frozen, (0, 2, 3), dtype))
        pre = f"rpn/deconv{b + 1}"
        u = Fn.conv_transpose2d(x, t[pre + "/kernel"].permute(3, 2, 0, 1), stride=d.upsample_strides[b])
        ups.append(torch.relu(_bn(u, t, w, pre + "/bn", pre in frozen, (0, 2, 3), dtype)))
    cat = torch.cat(ups, dim=1)

    def head(name):
        return Fn.conv2d(cat, t[name + "/kernel"].permute(3, 2, 0, 1), bias=t[name + "/bias"]).permute(0, 2, 3, 1)

    use_dir = bool(d.config["model"]["second"]["use_direction_classifier"])
    box, cls = head("rpn/conv_box"), head("rpn/conv_cls")
    dr = head("rpn/conv_dir_cls") if use_dir else None
    lt = loss_ref.loss_tensors(d.config["model"]["second"], box, cls, dr, labels, reg_targets, anchors, dtype)
    lt["loss"].backward()
    vals = {k: float(v.detach()) for k, v in lt.items() if k != "num_positives"}
    vals["num_positives"] = int(lt["num_positives"])
    grads = {k: (tt.grad.numpy() if tt.grad is not None else np.zeros(tt.shape, np.float32))
             for k, tt in t.items() if tt.requires_grad}
    return vals, grads
