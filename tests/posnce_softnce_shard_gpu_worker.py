"""Worker of tests/test_posnce_softnce_distributed_gpu.py: two or three ranks sharing the box's one GPU over gloo, the
study-positive and the soft-target InfoNCE of the global batch (distributed.global_batch_study_positive_infonce /
distributed_label_targets.global_batch_soft_target_infonce) on the product's HIP ops.  Each rank checks its rows against
  (a) the single-process one-call step on the full batch (study_positives.study_positive_infonce /
      soft_targets.soft_target_infonce): the same kernels and operand rounding, only the summation order of the merges
      and of dY / the parameter gradients differs -> the figures of tests/nce_shard_gpu_worker.py, for its reasons: 3e-5
      relative; the gradients of the bilinear critic in bf16 at 2e-3 (a row block's dT is summed in another order before
      it is rounded to bf16); the separable critic in bf16 at 6e-3 (a rank rounds ITS partial dC to bf16);
  (b) the fp64 restatements (tests/posnce_reference.py, tests/softnce_reference.py) through ``_check`` of
      tests/test_posnce_gpu.py and tests/test_softnce_gpu.py, on the rank's rows;
and that every rank holds bit-identical loss and lse_cols, that two identical steps give identical bits and that a
forward under torch.no_grad() gives the same loss.  Unique ids (study positives) and mix = 0 (soft targets) are also held
against the sharded per-sample InfoNCE, distributed.global_batch_mi_bound(..., "infonce_symmetric"), at the tolerances of
tests/test_posnce_gpu.py::test_unique_ids_give_the_per_sample_infonce.
Every comparison prints "<error / tolerance>" before it asserts."""
import math
import os
import sys

import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "mutual-information-multimodal_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from nce_shard_gpu_worker import ids  # noqa: E402


def masks(pattern, b):
    """int64 [b] finding-set masks; every pattern but "empty" has similar reports on different ranks."""
    gen = torch.Generator().manual_seed(1000 + b)
    if pattern == "random14":
        return torch.randint(0, 1 << 14, (b,), generator=gen, dtype=torch.int64)
    if pattern == "study":        # one bit per study; samples i, i + 50, i + 100, ... are one study
        return torch.ones(b, dtype=torch.int64) << (torch.arange(b, dtype=torch.int64) % 50)
    if pattern == "equal":
        return torch.full((b,), 0x2a51, dtype=torch.int64)
    if pattern == "empty":
        return torch.zeros(b, dtype=torch.int64)
    raise ValueError(pattern)


def cases(world):
    """(loss, critic, precision, b, d, mode, pattern, tau, mix).  World 2: B = 256 on the 16-bit chain, B = 192 with
    b_rows = 96 (the diagonal straddles two column tiles), B = 200, d = 60 on the generic kernels in bf16.  World 3:
    B = 192 (b_rows = 64) and B = 288 (b_rows = 96).  "unique" / mix = 0 also run against the per-sample InfoNCE."""
    if world == 2:
        return [("pos", "bilinear", "bf16", 256, 128, 1, "dup_across", None, None),
                ("pos", "bilinear", "bf16", 192, 64, 1, "majority", None, None),
                ("pos", "bilinear", "bf16", 200, 60, 1, "dup_across", None, None),
                ("pos", "bilinear", "f32", 192, 64, 0, "dup_in_rank", None, None),
                ("pos", "separable", "bf16", 256, 128, 1, "dup_across", None, None),
                ("pos", "separable", "f32_exact", 192, 64, 0, "all_equal", None, None),
                ("pos", "bilinear", "bf16", 256, 128, 1, "unique", None, None),
                ("soft", "bilinear", "bf16", 256, 128, 1, "random14", 0.5, 0.5),
                ("soft", "bilinear", "bf16", 192, 64, 1, "study", 0.1, 1.0),
                ("soft", "bilinear", "bf16", 200, 60, 0, "random14", 0.5, 1.0),
                ("soft", "bilinear", "f32", 192, 64, 1, "random14", 0.5, 0.5),
                ("soft", "separable", "bf16", 256, 128, 1, "equal", 0.5, 1.0),
                ("soft", "separable", "f32", 192, 64, 1, "random14", 0.1, 0.5),
                ("soft", "bilinear", "bf16", 192, 64, 1, "random14", 0.5, 0.0)]
    return [("pos", "bilinear", "bf16", 192, 64, 1, "dup_across", None, None),
            ("pos", "bilinear", "f32", 288, 64, 0, "majority", None, None),
            ("pos", "separable", "bf16", 288, 64, 1, "dup_in_rank", None, None),
            ("pos", "bilinear", "f32", 192, 64, 1, "unique", None, None),
            ("soft", "bilinear", "bf16", 288, 64, 1, "random14", 0.5, 0.5),
            ("soft", "bilinear", "f32_exact", 192, 64, 0, "empty", 0.5, 1.0),
            ("soft", "separable", "bf16", 192, 64, 1, "study", 0.1, 1.0),
            ("soft", "bilinear", "bf16", 288, 64, 1, "random14", 0.5, 0.0)]


def _ratio(what, err, tol):
    print(f"shard-err {what} {err / tol:.3f}", flush=True)
    assert err <= tol, (what, err, tol)


def _allclose(what, got, want, rtol, atol):
    """torch.allclose with the figure printed first."""
    ratio = float(((got - want).abs() / (atol + rtol * want.abs())).max())
    print(f"shard-err {what} {ratio:.3f}", flush=True)
    assert ratio <= 1.0, (what, ratio)


def main():
    import posnce_reference as pref
    import softnce_reference as sref
    import test_posnce_gpu as tpg
    import test_softnce_gpu as tsg
    from mutual_info_img_txt import distributed as mid, distributed_label_targets as mlt, soft_targets, study_positives
    from mutual_info_img_txt.model import BilinearCritic, SeparableCritic
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    dev = torch.device("cuda:0")
    for loss_kind, kind, prec, b, d, mode, pattern, tau, mix in cases(world):
        est = ("infonce_rowwise", "infonce_symmetric")[mode]
        sym = mode == 1
        br = b // world
        rows = slice(rank * br, (rank + 1) * br)
        gen = torch.Generator().manual_seed(b * 5 + d)
        x = torch.randn(b, d, generator=gen)
        y = torch.randn(b, d, generator=gen)
        if kind == "bilinear":
            critic = BilinearCritic(d, d)
            with torch.no_grad():
                critic.weight.copy_(torch.randn(d, d, generator=gen) * (0.3 / math.sqrt(d)))
            pnames = ["dw"]
        else:
            k = 48
            critic = SeparableCritic(d, d, k)
            with torch.no_grad():
                critic.wg.copy_(torch.randn(d, k, generator=gen) * (0.7 / math.sqrt(d)))
                critic.wh.copy_(torch.randn(d, k, generator=gen) * (0.7 / math.sqrt(d)))
            pnames = ["dwg", "dwh"]
        host_params = [p.detach().clone() for p in critic.parameters()]
        critic = critic.to(dev)
        xd, yd = x.to(dev), y.to(dev)
        pos = loss_kind == "pos"
        codes_host = ids(pattern, b, br) if pos else masks(pattern, b)
        codes = codes_host.to(dev)
        extra = "n_pos" if pos else "target_norm"
        params = [p.detach() for p in critic.parameters()]
        tag = f"world {world} rank {rank} {loss_kind} {kind} {prec} B={b} d={d} {est} {pattern} {tau} {mix}"

        # (a) single process, full batch, one call
        xr, yr = xd.clone().requires_grad_(True), yd.clone().requires_grad_(True)
        for p in critic.parameters():
            p.grad = None
        if pos:
            ref_loss, ref_st = study_positives.study_positive_infonce(xr, yr, codes, critic, symmetric=sym, precision=prec,
                                                                      return_stats=True)
        else:
            ref_loss, ref_st = soft_targets.soft_target_infonce(xr, yr, codes, critic, tau=tau, mix=mix, symmetric=sym,
                                                                precision=prec, return_stats=True)
        ref_loss.backward()
        ref_grads = [xr.grad[rows], yr.grad[rows]] + [p.grad.clone() for p in critic.parameters()]
        tol = 6e-3 if (kind == "separable" and prec == "bf16") else 3e-5
        gtol = max(tol, 2e-3) if prec == "bf16" else tol

        def step():
            xl, yl = xd[rows].clone().requires_grad_(True), yd[rows].clone().requires_grad_(True)
            pl = [p.clone().requires_grad_(True) for p in params]
            if pos:
                loss, st = mid.global_batch_study_positive_infonce(xl, yl, codes[rows].contiguous(), pl, symmetric=sym,
                                                                   precision=prec, critic=kind, return_stats=True)
            else:
                loss, st = mlt.global_batch_soft_target_infonce(xl, yl, codes[rows].contiguous(), pl, tau=tau, mix=mix,
                                                                symmetric=sym, precision=prec, critic=kind,
                                                                return_stats=True)
            assert loss.shape == () and st["lse_rows"].shape == (br,) and st["lse_cols"].shape == (b,)
            assert st[extra].shape == (br,)
            loss.backward()
            torch.cuda.synchronize()
            return loss.detach(), st, [xl.grad, yl.grad] + [p.grad for p in pl]

        loss, st, grads = step()
        _ratio(f"{tag} (a) loss", abs(float(loss) - float(ref_loss)), tol * max(1.0, abs(float(ref_loss))))
        for name, got, want in [("lse_rows", st["lse_rows"], ref_st["lse_rows"][rows]),
                                ("lse_cols", st["lse_cols"], ref_st["lse_cols"])]:
            _ratio(f"{tag} (a) {name}", float((got - want).abs().max()) / max(1.0, float(want.abs().max())), tol)
        if pos:
            assert torch.equal(st["n_pos"], ref_st["n_pos"][rows]), tag
        else:  # the same kernel on the same gathered masks
            assert torch.equal(st["target_norm"], ref_st["target_norm"][rows]), tag
        for n, (got, want) in enumerate(zip(grads, ref_grads)):
            wmax = float(want.abs().max())
            if wmax == 0.0:
                assert float(got.abs().max()) == 0.0, tag
                continue
            _ratio(f"{tag} (a) grad{n}", float((got - want).abs().max()) / wmax, gtol)

        # (b) the fp64 restatement, on the rank's rows
        rounded = prec == "bf16"
        if pos and kind == "bilinear":
            o = pref.bilinear_case(x, y, host_params[0], codes_host.tolist(), est, rounded=rounded)
        elif pos:
            o = pref.separable_case(x, y, host_params[0], host_params[1], codes_host.tolist(), est, rounded=rounded)
        elif kind == "bilinear":
            o = sref.bilinear_case(x, y, host_params[0], codes_host, est, tau, mix, rounded=rounded)
        else:
            o = sref.separable_case(x, y, host_params[0], host_params[1], codes_host, est, tau, mix, rounded=rounded)
        o = dict(o)
        for name in ("lse_rows", "dx", "dy", extra):
            o[name] = o[name][rows]
        got = {"loss": loss, "lse_rows": st["lse_rows"], "lse_cols": st["lse_cols"], extra: st[extra], "dx": grads[0],
               "dy": grads[1], **dict(zip(pnames, grads[2:]))}
        (tpg if pos else tsg)._check(got, o, ["dx", "dy"] + pnames, prec, f"{tag} (b)")

        # every rank: identical loss and lse_cols bits
        mine = torch.cat([loss.reshape(1), st["lse_cols"]]).cpu()
        every = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        assert all(torch.equal(e, every[0]) for e in every), tag
        # a second identical step: identical bits
        loss2, st2, grads2 = step()
        assert torch.equal(loss2, loss) and all(torch.equal(st2[n], st[n]) for n in st), tag
        assert all(torch.equal(g2, g) for g2, g in zip(grads2, grads)), tag
        # forward only
        with torch.no_grad():
            if pos:
                l3 = mid.global_batch_study_positive_infonce(xd[rows].clone(), yd[rows].clone(), codes[rows].contiguous(),
                                                             params, symmetric=sym, precision=prec, critic=kind)
            else:
                l3 = mlt.global_batch_soft_target_infonce(xd[rows].clone(), yd[rows].clone(), codes[rows].contiguous(),
                                                          params, tau=tau, mix=mix, symmetric=sym, precision=prec,
                                                          critic=kind)
        torch.cuda.synchronize()
        assert not l3.requires_grad and torch.equal(l3, loss), tag

        # unique ids / mix = 0: the sharded per-sample InfoNCE
        if pattern == "unique" or mix == 0.0:
            assert sym
            xl, yl = xd[rows].clone().requires_grad_(True), yd[rows].clone().requires_grad_(True)
            pl = [p.clone().requires_grad_(True) for p in params]
            sid = torch.arange(b, dtype=torch.int64, device=dev)
            full, (r, c) = mid.global_batch_mi_bound(xl, yl, sid[rows].contiguous(), pl, "infonce_symmetric", prec,
                                                     critic=kind, return_stats=True)
            full.backward()
            torch.cuda.synchronize()
            _allclose(f"{tag} nce loss", loss, full.detach(), 1e-5, 3e-5)
            _allclose(f"{tag} nce lse_rows", st["lse_rows"], r, 1e-5, 3e-5)
            _allclose(f"{tag} nce lse_cols", st["lse_cols"], c, 1e-5, 3e-5)
            if pos:
                assert int(st["n_pos"].min()) == 1 and int(st["n_pos"].max()) == 1
            for n, (g, w) in enumerate(zip(grads, [xl.grad, yl.grad] + [p.grad for p in pl])):
                _allclose(f"{tag} nce grad{n}", g, w, 2e-3, 3e-4 * float(w.abs().max()))
        dist.barrier()
        if rank == 0:
            print(f"posnce softnce shard gpu ok: {tag}", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
