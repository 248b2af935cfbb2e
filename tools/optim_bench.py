"""Time of one optimizer step on the headline parameter set, UNet(1, 8): 7.76 M parameters in 64 tensors, four ways,
alternating in one process, HIP events around `reps` steps each (no forward / backward: the gradient buffer is filled once).

  (a) FusedAdamW.step()                                     one launch                 28 B per element
  (b) FusedAdamW(max_grad_norm=...).step()                  three launches, no sync    32 B per element
  (c) torch.optim.AdamW(fused=True).step() on the 64 tensors, and (c') the same after clip_grad_norm_(foreach=True)
  (d) FusedSGD(momentum=0.9).step()                         what the step costs today  20 B per element

Prints one JSON line: per form the median over `rounds` windows and their spread (max - min) in microseconds per step, the
bandwidth floor bytes / HBM rate and the achieved bytes/s.  The four flat buffers of (a) total 4 x 31 MB: less than the last-level
cache, so the achieved rate may exceed what HBM alone delivers -- it is reported as it is.

usage: optim_bench.py [reps] [rounds]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from retinal_oct_image_segmentation_via_deep_learning_amd.SOTAS.Lesions_Segment.YNet_2022 import UNet  # noqa: E402
from retinal_oct_image_segmentation_via_deep_learning_amd.optim import NO_DECAY_1D, FusedAdamW, FusedSGD  # noqa: E402

HBM_BYTES_PER_S = 6.29e12   # measured float4 copy rate (8.0 TB/s is the specification)
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
MAX_NORM = 1.0


def model_with_grads(seed):
    torch.manual_seed(seed)
    m = UNet(1, 8).cuda().train()
    gen = torch.Generator(device="cuda").manual_seed(seed + 1)
    return m, gen


def fill(params, gen):
    for p in params:
        p.grad.copy_(torch.randn(p.shape, generator=gen, device="cuda") * 1e-2)


def window(step):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps      # microseconds per step


def main():
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench.py needs a GPU: nothing is measured without one")
    forms = {}
    m, gen = model_with_grads(1)
    opt_a = FusedAdamW(list(m.named_parameters()), lr=1e-3, no_decay=NO_DECAY_1D)
    fill(opt_a.params, gen)
    total, n_params = opt_a.flat_p.numel(), sum(p.numel() for p in opt_a.params)
    forms["a_fused_adamw"] = (opt_a.step, 28 * total)
    m, gen = model_with_grads(1)
    opt_b = FusedAdamW(list(m.named_parameters()), lr=1e-3, no_decay=NO_DECAY_1D, max_grad_norm=MAX_NORM)
    fill(opt_b.params, gen)
    forms["b_fused_adamw_clip"] = (opt_b.step, 32 * total)
    m, gen = model_with_grads(1)
    tparams = list(m.parameters())
    for p in tparams:
        p.grad = torch.zeros_like(p)
    fill(tparams, gen)
    opt_c = torch.optim.AdamW(tparams, lr=1e-3, fused=True)
    forms["c_torch_adamw_fused"] = (opt_c.step, 28 * n_params)

    def clipped():
        torch.nn.utils.clip_grad_norm_(tparams, MAX_NORM, foreach=True)
        opt_c.step()
    forms["c_torch_clip_adamw_fused"] = (clipped, 32 * n_params)
    m, gen = model_with_grads(1)
    opt_d = FusedSGD(list(m.named_parameters()), lr=0.01, momentum=0.9)
    fill(opt_d.params, gen)
    forms["d_fused_sgd"] = (opt_d.step, 20 * total)

    for step, _ in forms.values():          # warm-up: code objects, torch's lazily created state
        for _ in range(20):
            step()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(rounds):                 # alternating, so that a drift of the machine reaches every form alike
        for k, (step, _) in forms.items():
            times[k].append(window(step))
    out = {"params": n_params, "flat_total": total, "tensors": len(opt_a.params), "reps": reps, "rounds": rounds,
           "hbm_bytes_per_s": HBM_BYTES_PER_S, "forms": {}}
    for k, (_, nbytes) in forms.items():
        med = statistics.median(times[k])
        out["forms"][k] = {"us_per_step": round(med, 2), "spread_us": round(max(times[k]) - min(times[k]), 2),
                           "window_s": round(med * reps * 1e-6, 3), "bytes": nbytes,
                           "floor_us": round(nbytes / HBM_BYTES_PER_S * 1e6, 2),
                           "achieved_TB_per_s": round(nbytes / (med * 1e-6) / 1e12, 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
