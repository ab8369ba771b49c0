"""One minibatch of the local-SGD kernels (csrc/cfa_local_sgd.hip) is the gradient kernels'
gradient (csrc/cfa_grad.hip) applied on the host, bit for bit: both run the phases of
csrc/cfa_tf1_graph.h, and only where a parameter's sum goes differs.

``Engine.local_sgd`` with steps = 1 and batch_rows = B against ``Engine.grad_rows`` on the same
rows and models without a workspace (one workgroup per evaluation, no batch split; B samples are
one LDS chunk), then ``W - np.float32(lr) * G`` in numpy fp32: the product and the difference each
round once, as the kernel's do with contraction off. Three devices with their own data, the
smallest shapes that reach each shared path."""
import numpy as np
import pytest
import torch

from test_gpu_local_training import CNN_ODD, LR, NAMES, NN_TINY, _cuda, _data, _kernel_geom, _layout, _run

pytestmark = pytest.mark.gpu

K_BLOCK, K_SPAN = 512, 32  # kGradBlock, kSpan

# name: (ml, geometry, B)
CASES = {
    # L is no multiple of the stride: boundary windows on the branch-free <16, 5> path
    "cnn_16_5": (1, {"filter": 16, "number": 8, "stride": 5, "input_data": 37, "classes": 5}, 4),
    "cnn_runtime_loops": (1, CNN_ODD, 3),
    "2nn_slice_in_registers": (2, NN_TINY, 3),
    # G * H = 600 > 512 threads; at these sizes d z sits 12 bytes past a 16-byte boundary in the
    # gradient kernel's LDS plan, so its W1 sums take the scalar loop
    "2nn_memory_fallback": (2, {"intermediate_nodes": 200, "input_data": 70, "classes": 3}, 2),
    # the same with C = 4: d z is 16-byte aligned and the gradient kernel's W1 sums go four at a time
    "2nn_memory_fallback_float4": (2, {"intermediate_nodes": 200, "input_data": 70, "classes": 4}, 2),
}


def _path(ml, geom, B):
    """What puts a case on its path, from the launch plans of the two files."""
    L, C = geom["input_data"], geom["classes"]
    if ml == 1:
        fast = (geom["filter"], geom["stride"]) == (16, 5)
        return {"fast": fast, "taps_in_regs": geom["filter"] <= 32 and K_BLOCK % geom["number"] == 0,
                "L % S": L % geom["stride"]}
    H = geom["intermediate_nodes"]
    G = -(-L // K_SPAN)
    dz_floats = H + H * C + C + B * L + B * H  # b1 W2 b2 xs act come before dz (Bc = B)
    return {"w_in_regs": G * H <= K_BLOCK, "float4": H % 4 == 0 and dz_floats % 4 == 0}


EXPECTED = {
    "cnn_16_5": {"fast": True, "taps_in_regs": True, "L % S": 2},
    "cnn_runtime_loops": {"fast": False, "taps_in_regs": False, "L % S": 1},
    "2nn_slice_in_registers": {"w_in_regs": True, "float4": False},
    "2nn_memory_fallback": {"w_in_regs": False, "float4": False},
    "2nn_memory_fallback_float4": {"w_in_regs": False, "float4": True},
}


@pytest.mark.parametrize("name", list(CASES))
def test_one_step_is_the_gradient_applied_on_the_host(gpu, name):
    ml, geom, B = CASES[name]
    assert _path(ml, geom, B) == EXPECTED[name]
    D = 3
    x, y, W = _data(11, ml, geom, D, B)
    _, offs = _layout(ml, geom)
    P = offs[4]
    rows = torch.arange(D, dtype=torch.int32, device="cuda")
    grads = torch.full((D, P), float("nan"), device="cuda")
    gpu.grad_rows(ml, _cuda(x), _cuda(y), _cuda(W), rows, rows, grads, _kernel_geom(geom))
    torch.cuda.synchronize()
    G = grads.cpu().numpy()
    want = W - np.float32(LR) * G
    assert want.dtype == np.float32
    got, padding, _ = _run(gpu, ml, geom, x, y, W, B, B, 1)
    assert np.all(padding == 7.5)
    for k in range(4):
        a, w = got[:, offs[k]:offs[k + 1]], want[:, offs[k]:offs[k + 1]]
        differ = int(np.count_nonzero(a.view(np.uint32) != w.view(np.uint32)))
        moved = int(np.count_nonzero(a != W[:, offs[k]:offs[k + 1]]))
        print(f"{name} {NAMES[k]}: {differ} of {a.size} words differ, {moved} moved by the step")
        assert differ == 0 and moved > 0, (name, NAMES[k], differ, moved)
