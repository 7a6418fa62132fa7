#!/usr/bin/env python3
"""Wall time of Newton steps with ALL device work on partitioned levels (alfi_amd.dist.DistNavierStokesSolver): the operator
refresh of every rank's own rows on the device (alfi_level_set_assembly on partitioned levels), the outer Krylov loop inside
the library (alfi_saddle_solve on a partitioned finest level).  Several ranks share the box's one GPU through the shared-memory
stand-in for librccl (tests/mock_rccl), so the times are FUNCTIONAL (one GPU does the work of N), not a scaling measurement.

    python scripts/dist_newton_time.py cfg4 --ranks 4 --re 10 100
    python scripts/dist_newton_time.py cfg5s --ranks 2 --burman 5e-3 --compare
    python scripts/dist_newton_time.py cfg5s --ranks 2 --host-state
    python scripts/dist_newton_time.py cfg2 --ranks 2 --adjoint --compare

Every config runs with the Newton state distributed on the devices -- the Scott-Vogelius ones (cfg5s, cfg5: the structured
bfs3d stand-in) included, their coarse levels' states being weighted gathers of the exchanged finest velocity; --host-state
selects the replicated host state instead (device_state=False: every level's state formed on the host and uploaded, residual
and update gathered through the host), for comparisons.  Next to the times, every rank's bytes across PCIe per Newton step
(alfi_transfer_stats: every copy the library makes, the larger direction).  --burman WEIGHT adds the interior-penalty term
(every rank over the facets of its cells) and reports its per-rank cost: the refresh of all levels with and without the term
and the term's residual pass on the finest level.

The parent never touches the GPU: it starts the rank processes and relays rank 0's report; host assemblies during the Newton
loops are counted (must be 0) and the Newton / Krylov counts printed next to the single-GPU solver's when --compare is given."""
import argparse
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rank_main(args):
    import numpy as np
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    import bench
    from alfi_amd import _hostlib
    from alfi_amd.dist import DistNavierStokesSolver
    from alfi_amd.problem import TwoDimLidDrivenCavityProblem, ThreeDimLidDrivenCavityProblem
    prob, nref, ke, kw = problem_and_options(args)
    t0 = time.time()
    s = DistNavierStokesSolver(prob, nref, ke, min_dofs=args.min_dofs, device_state=not args.host_state, **kw)
    if rank == 0:
        print("%s on %d ranks (transport %s): %d velocity + %d pressure dofs, setup %.1f s, device assembly %s, state %s, "
              "levels on this rank %d.." % (args.config, world, s.dmg.transport, s.n_u, s.n_p, time.time() - t0,
                                            s.device_assembly, "distributed on the devices" if s._device_state_resident()
                                            else "replicated on the hosts", s.dmg.lmin), flush=True)
    calls = []
    real, real_supg, real_burman = _hostlib.assemble_bsr, _hostlib.supg, _hostlib.burman
    _hostlib.assemble_bsr = lambda *a, **kw: (calls.append(1), real(*a, **kw))[1]
    _hostlib.supg = lambda *a, **kw: (calls.append(1), real_supg(*a, **kw))[1]
    _hostlib.burman = lambda *a, **kw: (calls.append(1), real_burman(*a, **kw))[1]
    for re in args.re:
        for kk in s.timings:
            s.timings[kk] = 0 if kk == "newton_steps" else 0.0
        dist.barrier()
        s.ctx.transfer_stats(reset=True)
        t0 = time.time()
        _, info = s.solve(re)
        wall = time.time() - t0
        n = max(s.timings["newton_steps"], 1)
        pcie = [None] * world
        dist.all_gather_object(pcie, max(s.ctx.transfer_stats()) // n)
        if rank == 0:
            print("Re %g: %d Newton steps, %d Krylov its, converged %s, wall %.2f s = %.2f s per Newton step "
                  "(assemble %.3f, factor %.3f, residual %.3f, solve %.3f per step); host assemblies so far: %d"
                  % (re, info["nonlinear_iter"], info["linear_iter"], info["converged"], wall, wall / n,
                     s.timings["assemble_s"] / n, s.timings["factor_s"] / n, s.timings["residual_s"] / n,
                     s.timings["solve_s"] / n, len(calls)), flush=True)
            print("Re %g: bytes across PCIe per Newton step, per rank: %s" % (re, pcie), flush=True)
        if args.adjoint:              # COLLECTIVE: every rank solves its part (the transposed refresh of its own rows)
            from newton_step_time import adjoint_functional, adjoint_line
            ainfo = s.solve_adjoint(adjoint_functional(s))[1]
            if rank == 0:
                print(adjoint_line(re, ainfo), flush=True)
    got = [None] * world
    dist.all_gather_object(got, len(calls))
    if rank == 0:
        print("host assemblies during the Newton loops, per rank:", got, flush=True)
    if args.burman is not None and s.device_assembly:
        cost = burman_cost(s)
        every = [None] * world
        dist.all_gather_object(every, cost)
        if rank == 0:
            for r, (t_plain, t_burman, t_res, nf) in enumerate(every):
                print("rank %d: refresh of its levels %.2f ms without, %.2f ms with the Burman term (%d facets); Burman residual "
                      "pass on the finest level %.2f ms" % (r, 1e3 * t_plain, 1e3 * t_burman, nf, 1e3 * t_res), flush=True)
    s.close()
    dist.barrier()
    dist.destroy_process_group()


def problem_and_options(args):
    """(problem, nref, element degree, solver keywords) of a bench config and the stabilisation options."""
    import bench
    from alfi_amd.problem import TwoDimLidDrivenCavityProblem, ThreeDimLidDrivenCavityProblem
    dim, baseN, nref, ke, Re, k = bench.CONFIGS[args.config]
    if args.supg is not None and args.burman is not None:
        raise SystemExit("--supg and --burman exclude each other")
    if dim == "sv":
        if isinstance(baseN, str):
            raise SystemExit("the unstructured-mesh configs are not set up here")
        from alfi_amd.problem import ThreeDimBackwardsFacingStepProblem
        kw = dict(discretisation="sv")
        if args.burman is not None:
            kw.update(stabilisation_type="burman", stabilisation_weight=args.burman)
        elif args.supg is not None:
            raise SystemExit("--supg is for the P0-pressure configs")
        return ThreeDimBackwardsFacingStepProblem(baseN), nref, ke, kw
    if args.burman is not None:
        raise SystemExit("--burman is for the Scott-Vogelius configs (cfg5s, cfg5)")
    prob = TwoDimLidDrivenCavityProblem(baseN) if dim == 2 else ThreeDimLidDrivenCavityProblem(baseN)
    return prob, nref, ke, dict(stabilisation_type="supg" if args.supg is not None else None, stabilisation_weight=args.supg)


def burman_cost(s, reps=5):
    """Seconds per call on this rank, about the final state at adv = 1: the refresh of all its levels without and with the
    Burman term, and the term's residual pass on the finest level; and the number of facets of its finest level."""
    import time
    s._upload_states(s.u)
    lv = [(dl, asm[1]) for asm, dl in zip(s._asm, s.dmg.levels) if asm is not None]

    def timed(fn):
        with s._on_stream():
            fn()
            s.dmg.sync()
            t0 = time.time()
            for _ in range(reps):
                fn()
            s.dmg.sync()
        return (time.time() - t0) / reps

    t_plain = timed(lambda: [dl.assemble(s.nu, s.gamma, 1.0, st, True) for dl, st in lv])
    t_burman = timed(lambda: [dl.assemble_burman(s.nu, s.gamma, 1.0, st, s.burman_weight, True) for dl, st in lv])
    fin, st = lv[-1]
    t_res = timed(lambda: fin.burman(s.burman_weight, st, False, s._dres))
    return t_plain, t_burman, t_res, int(s._facet_parts[s.dmg.local_levels[-1].level].table.nf)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("--ranks", type=int, default=4)
    ap.add_argument("--re", type=float, nargs="+", default=[10.0, 100.0])
    ap.add_argument("--min-dofs", type=int, default=None,
                    help="levels below this many dofs live on rank 0 (default 400000; 1 for the Scott-Vogelius configs, whose "
                         "levels are smaller)")
    ap.add_argument("--supg", type=float, default=None, metavar="WEIGHT",
                    help="SUPG stabilisation with this weight (the reference's production runs: 0.05)")
    ap.add_argument("--burman", type=float, default=None, metavar="WEIGHT",
                    help="Burman stabilisation of the Scott-Vogelius configs with this weight (the reference's run lines: 5e-3)")
    ap.add_argument("--host-state", action="store_true",
                    help="the Newton state replicated on the hosts (device_state=False), for comparisons")
    ap.add_argument("--adjoint", action="store_true",
                    help="one adjoint solve after every forward solve: refresh / factor / solve seconds and the Krylov count "
                         "(with --compare next to the single-GPU solver's)")
    ap.add_argument("--compare", action="store_true", help="also run the single-GPU solver (counts side by side)")
    ap.add_argument("--rank-process", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.min_dofs is None:
        import bench
        args.min_dofs = 1 if bench.CONFIGS[args.config][0] == "sv" else 400000
    if args.rank_process:
        return rank_main(args)
    from tests.mock_rccl.build import build
    lib = build()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    # the host cores this job may use (OMP_NUM_THREADS where it is set: a share of a larger machine), split over the ranks
    threads = max(1, int(os.environ.get("OMP_NUM_THREADS") or os.cpu_count() or 8) // args.ranks)
    for r in range(args.ranks):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(args.ranks), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), OMP_NUM_THREADS=str(threads), ALFI_HOST_THREADS=str(threads),
                   ALFI_DIST_TRANSPORT="rccl", ALFI_RCCL_LIB=lib)
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), args.config, "--ranks", str(args.ranks),
                                       "--min-dofs", str(args.min_dofs), "--rank-process"] +
                                      (["--supg", str(args.supg)] if args.supg is not None else []) +
                                      (["--burman", str(args.burman)] if args.burman is not None else []) +
                                      (["--host-state"] if args.host_state else []) +
                                      (["--adjoint"] if args.adjoint else []) +
                                      ["--re"] + [str(x) for x in args.re], env=env, cwd=ROOT))
    done = False
    try:
        # a rank that fails leaves the others waiting in a collective: end them with it
        while any(p.poll() is None for p in procs) and not any(p.poll() for p in procs):
            time.sleep(0.2)
        done = not any(p.poll() for p in procs)
    finally:
        for p in procs:
            if not done and p.poll() is None:
                p.kill()
    rc = [p.wait() for p in procs]
    if any(rc):
        raise SystemExit("rank exit codes %s" % rc)
    if args.compare:
        subprocess.check_call([sys.executable, os.path.join(ROOT, "scripts", "newton_step_time.py"), args.config] +
                              (["--supg", str(args.supg)] if args.supg is not None else []) +
                              (["--burman", str(args.burman)] if args.burman is not None else []) +
                              (["--adjoint"] if args.adjoint else []) +
                              ["--re"] + [str(x) for x in args.re], cwd=ROOT)


if __name__ == "__main__":
    main()
