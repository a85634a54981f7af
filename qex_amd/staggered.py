"""Host-side mirror of QEX's staggered operator / solver interface over the C ABI.

Same names, argument meaning and error behaviour as the reference so that tests read like
QEX's own (tests/examples/testStagProp.nim, src/physics/stagSolve.nim:516-680):

    newStag(g) / newStag3(g, g3)      src/physics/stagD.nim:522-564
    Staggered.D / Ddag                src/physics/stagD.nim:566-571
    Staggered.eoReconstruct           src/physics/stagD.nim:583-586
    stagD2 / stagD2ee / stagD2oo      src/physics/stagD.nim:349-395,463-469
    Staggered.solveEE / solveOO       src/physics/stagSolve.nim:134-138
    Staggered.solve (single / multi)  src/physics/stagSolve.nim:224-294,347-446
    SolverParams                      src/solvers/solverBase.nim:10-58

Fields are numpy arrays in the V=1 even-odd host format (qex_amd.layout).  All arithmetic
happens in libqexhip.so on the GPU; nothing here computes on field data.
"""
import ctypes as C
import time
import numpy as np

from . import _lib
from ._lib import check, lib

EVEN, ODD, ALL = 0, 1, 2
# SolverParams.sloppySolve (solverBase.nim:8-15): SloppyHalf runs single precision unless the context's option "half" is 1, which
# gives the single-system solves 16-bit storage, on one rank and on t-sharded lattices alike (Context.set_option("half", 1);
# half_pack_host is the format; sharded, the faces travel at 16 B per site).  Lock-step batches of a sharded context are refused
# unless its option "batch_ranks" is 1 (then fp32, or 16-bit with "half_batch" = 1, as on one rank); its multi-shift solves refine
# one shift at a time in single precision
SloppyNone, SloppySingle, SloppyHalf = 0, 1, 2
_SUBSET = {"even": EVEN, "odd": ODD, "all": ALL}


def _p(a):
    if a is None:
        return None
    if a.dtype != np.float64 or not a.flags["C_CONTIGUOUS"]:
        raise ValueError("fields must be C-contiguous float64 arrays")
    return a.ctypes.data_as(C.c_void_p)


def _ptrs(arrays):
    """the C array of the fields' addresses (a `double *const *` argument)"""
    return (C.c_void_p * len(arrays))(*[_p(a).value for a in arrays])


class SolverParams:
    """solverBase.nim:10-58 (fields the staggered path uses)."""

    def __init__(self, r2req=1e-6, maxits=50000, verbosity=1, usePrevSoln=False, sloppySolve=SloppyNone):
        self.r2req = r2req
        self.maxits = maxits
        self.verbosity = verbosity
        self.usePrevSoln = usePrevSoln
        self.sloppySolve = sloppySolve
        self.subsetName = "all"
        self.resetStats()

    def resetStats(self):
        self.calls = 0
        self.iterations = 0
        self.iterationsMax = 0
        self.seconds = 0.0
        self.flops = 0.0
        self.r2 = 0.0
        self.r2hist = None
        self.reliableUpdates = 0   # mixed-precision solves (sloppySolve != 0): fp64 true-residual updates
        self.refineIterations = []  # mixed-precision multi-shift solveXX: fp32 iterations spent refining each shift

    @property
    def finalIterations(self):
        return self.iterations

    def getStats(self):
        gf = 1e-9 * self.flops / self.seconds if self.seconds > 0 else 0.0
        return f"its: {self.iterations}  secs: {self.seconds:.6g}  Gf/s: {gf:.6g}  r2: {self.r2:.6g}"


def device_count():
    """HIP devices this process can bind (qexhip_device_count): a host picks device = (rank on its node) mod this count"""
    n = C.c_int(0)
    check(lib().qexhip_device_count(C.byref(n)))
    return int(n.value)


class Context:
    """One GPU / one rank (qexhip_init).  rank_geom must be (1,1,1,N)."""

    def __init__(self, lat_local, device=0, rank_geom=(1, 1, 1, 1), rank_coord=(0, 0, 0, 0)):
        self.lat = [int(v) for v in lat_local]
        self.vol = int(np.prod(self.lat))
        self._h = C.c_void_p()
        i4 = C.c_int * 4
        check(lib().qexhip_init(C.byref(self._h), device, i4(*self.lat), i4(*rank_geom), i4(*rank_coord)))
        self.rank_geom = tuple(rank_geom)
        self.rank_coord = tuple(rank_coord)

    def close(self):
        if self._h:
            lib().qexhip_finalize(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        buf = C.create_string_buffer(512)
        check(lib().qexhip_device_info(self._h, buf, 512))
        return buf.value.decode()

    def sync(self):
        check(lib().qexhip_sync(self._h))

    # communicator
    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        check(lib().qexhip_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, uid, nranks, rank):
        check(lib().qexhip_comm_init(self._h, uid, nranks, rank))

    def comm_info(self):
        """(nranks, rank, device, pci bus id) as RCCL / HIP report them; nranks = 0 without a communicator"""
        n, r, d = C.c_int(0), C.c_int(0), C.c_int(0)
        bus = C.create_string_buffer(64)
        check(lib().qexhip_comm_info(self._h, C.byref(n), C.byref(r), C.byref(d), bus, 64))
        return n.value, r.value, d.value, bus.value.decode()

    def comm_transport(self):
        """("none" | "rccl" | "peer", {exchanges, allreduces, arena_allocs, arena_bytes}) -- which transport comm_init chose"""
        buf = C.create_string_buffer(16)
        st = (C.c_long * 4)()
        check(lib().qexhip_comm_transport(self._h, buf, 16, st))
        return buf.value.decode(), dict(zip(("exchanges", "allreduces", "arena_allocs", "arena_bytes"), [int(v) for v in st]))

    def comm_count(self):
        """communicators held: 2 after comm_init (compute stream + overlapped face exchange), 1 with QEXHIP_COMM2=0"""
        n = C.c_int(0)
        check(lib().qexhip_comm_count(self._h, C.byref(n)))
        return n.value

    def sweep_info(self):
        """{"halo", "overlap", "interior_sites", "face_bytes"}: how a one-parity sweep is launched on this context"""
        o = (C.c_int * 8)()
        check(lib().qexhip_stag_sweep_info(self._h, o))
        r = {"halo": bool(o[0]), "overlap": bool(o[1]), "interior_sites": int(o[2]), "face_bytes": int(o[3]), "overlap_measured": bool(o[4]),
             "option_overlap": int(o[7])}
        if o[4]:
            r["measured_us_per_sweep"] = {"exchange_first": int(o[5]), "overlapped": int(o[6])}
        r.update(self.sweep_tuning())
        if o[4]:
            r["measured_us_per_sweep"]["fused"] = int(r["tuned_us_per_sweep"][2] + 0.5)
        return r

    def sweep_tuning(self):
        """what set_links measured and decided for the sweeps of a t-sharded slab (qexhip_stag_sweep_tuning)"""
        t = (C.c_double * 8)()
        check(lib().qexhip_stag_sweep_tuning(self._h, t))
        return {"exchange_us": float(t[0]), "boundary_at": float(t[1]), "tuned_us_per_sweep": [float(t[2]), float(t[3]), float(t[4])],
                "form": "fused" if int(t[5]) == 2 else "by_sites", "fused_spin_us": float(t[6])}

    def force_halo(self, on=True):
        check(lib().qexhip_comm_force_halo(self._h, 1 if on else 0))

    # timers
    def timers_enable(self, on=True):
        """on: False/0 off, True/1 every kernel class, 2 only the Dslash sweeps."""
        check(lib().qexhip_timers_enable(self._h, int(on)))

    def timers_reset(self):
        check(lib().qexhip_timers_reset(self._h))

    def set_option(self, name, value):
        check(lib().qexhip_set_option(self._h, name.encode(), int(value)))

    def timer(self, name):
        cnt, ms = C.c_long(0), C.c_double(0)
        check(lib().qexhip_timers_get(self._h, name.encode(), C.byref(cnt), C.byref(ms)))
        return cnt.value, ms.value

    # device-resident fields
    def field_new(self, host=None):
        fid = C.c_int(0)
        check(lib().qexhip_field_new(self._h, C.byref(fid)))
        if host is not None:
            check(lib().qexhip_field_upload(self._h, fid.value, _p(host)))
        return fid.value

    def field_free(self, fid):
        check(lib().qexhip_field_free(self._h, fid))

    def field_upload(self, fid, host):
        check(lib().qexhip_field_upload(self._h, fid, _p(host)))

    def field_download(self, fid):
        out = np.zeros((self.vol, 3, 2))
        check(lib().qexhip_field_download(self._h, fid, _p(out)))
        return out

    def field_zero(self, fid):
        check(lib().qexhip_field_zero(self._h, fid))

    def dev_dslash(self, r_id, x_id, parity, a=0.0, b=0.0):
        check(lib().qexhip_dev_dslash(self._h, r_id, x_id, parity, a, b))

    def dev_op_xx(self, r_id, x_id, m2, par_even=True):
        check(lib().qexhip_dev_op_xx(self._h, r_id, x_id, m2, 1 if par_even else 0))

    def dev_solve_xx(self, x_id, b_id, mass, r2req, maxits, par_even=True, histcap=0):
        its, fin = C.c_int(0), C.c_double(0)
        hist = np.zeros(max(histcap, 1))
        check(lib().qexhip_dev_solve_xx(self._h, x_id, b_id, mass, r2req, maxits, 1 if par_even else 0,
                                        C.byref(its), C.byref(fin), _p(hist), histcap))
        return its.value, fin.value, hist[: min(histcap, its.value + 1)]

    def dev_solve_xx_continue(self, x_id, r2req, maxits, histcap=0):
        """CgState re-entry (cg.nim:133 `if b2<0: # first call` not taken): go on iterating on the state the last dev_solve_xx
        on x_id left; maxits is the cumulative limit; returns (cumulative iterations, r2/b2, history from iteration 0)"""
        its, fin = C.c_int(0), C.c_double(0)
        hist = np.zeros(max(histcap, 1))
        check(lib().qexhip_dev_solve_xx_continue(self._h, x_id, float(r2req), int(maxits), C.byref(its), C.byref(fin), _p(hist), histcap))
        return its.value, fin.value, hist[: min(histcap, its.value + 1)]

    def dev_solve_xx_multi(self, x_ids, b_id, shifts, r2req, maxits, par_even=True, histcap=0, sloppy=None):
        """multi-shift solveXX on resident fields (stagSolve.nim:296-345); shifts[0] = base mass.  sloppy = 0, 1 or 2: the
        mixed-precision solve (qexhip_dev_solve_xx_multi_sloppy; no history), returning (fp32 iterations of phase 1, true r2/b2
        per shift, reliable updates, refinement iterations per shift)"""
        n = len(x_ids)
        its = C.c_int(0)
        if sloppy is not None:
            sloppy = _batch_sloppy(sloppy)
            if histcap > 0:
                raise ValueError("sloppy= with histcap > 0: the mixed-precision multi-shift solve keeps no residual history")
            fin, nup, ref = (C.c_double * n)(), C.c_int(0), (C.c_int * n)()
            check(lib().qexhip_dev_solve_xx_multi_sloppy(self._h, (C.c_int * n)(*[int(v) for v in x_ids]), int(b_id),
                                                         (C.c_double * n)(*[float(v) for v in shifts]), n, float(r2req), int(maxits),
                                                         1 if par_even else 0, sloppy, C.byref(its), fin, C.byref(nup), ref))
            return its.value, list(fin), nup.value, list(ref)
        hist = np.zeros(max(histcap, 1))
        check(lib().qexhip_dev_solve_xx_multi(self._h, (C.c_int * n)(*[int(v) for v in x_ids]), b_id,
                                              (C.c_double * n)(*[float(v) for v in shifts]), n, float(r2req), int(maxits),
                                              1 if par_even else 0, C.byref(its), _p(hist), histcap))
        return its.value, hist[: min(histcap, its.value + 1)]

    def dev_rational_xx(self, out_id, b_id, mass, f0, alpha, beta, r2req, maxits, par_even=True, histcap=0):
        """out[par] = r(M^+M) b[par] on resident fields, r(x) = f0 + sum_k alpha_k / (x + beta_k), M^+M = m^2 - D_eo D_oe: one
        accumulating multi-shift solve (qexhip_dev_rational_xx); returns (iterations, history of the base system)"""
        n = len(alpha)
        if len(beta) != n:
            raise ValueError("dev_rational_xx: %d residues, %d poles" % (n, len(beta)))
        its = C.c_int(0)
        hist = np.zeros(max(histcap, 1))
        check(lib().qexhip_dev_rational_xx(self._h, int(out_id), int(b_id), float(mass), float(f0), n,
                                           (C.c_double * n)(*[float(v) for v in alpha]), (C.c_double * n)(*[float(v) for v in beta]),
                                           float(r2req), int(maxits), 1 if par_even else 0, C.byref(its), _p(hist), histcap))
        return its.value, hist[: min(histcap, its.value + 1)]

    def dev_solve_xx_sloppy(self, x_id, b_id, mass, r2req, maxits, par_even=True, sloppy=SloppySingle):
        """mixed-precision solveXX on resident fields (qexhip_dev_solve_xx_sloppy); returns (fp32 iterations, true r2/b2,
        reliable updates)"""
        its, fin, nup = C.c_int(0), C.c_double(0), C.c_int(0)
        check(lib().qexhip_dev_solve_xx_sloppy(self._h, int(x_id), int(b_id), float(mass), float(r2req), int(maxits),
                                               1 if par_even else 0, int(sloppy), C.byref(its), C.byref(fin), C.byref(nup)))
        return its.value, fin.value, nup.value

    def dev_solve_xx_deflated(self, basis, nev, x_id, b_id, mass, r2req, maxits, sloppy=SloppyNone):
        """the deflated solveEE of hisqev.nim:653-705 on resident fields with the leading nev vectors of an EigBasis
        (qexhip_dev_solve_xx_deflated); returns (CG iterations, true |b - A x|^2/|b|^2)"""
        its, fin = C.c_int(0), C.c_double(0)
        check(lib().qexhip_dev_solve_xx_deflated(self._h, int(basis.id), int(nev), int(x_id), int(b_id), float(mass), float(r2req),
                                                 int(maxits), int(sloppy), C.byref(its), C.byref(fin)))
        return its.value, fin.value

    def dev_solve_xx_batch_deflated(self, basis, nev, x_ids, b_ids, masses, r2req, maxits, par_even=True, sloppy=SloppyNone):
        """the deflated lock-step batch on resident fields (qexhip_dev_solve_xx_batch_deflated): n <= 4 solveEE / solveOO with their
        own masses, both parities deflated from the even EigBasis with its leading nev vectors (None: basis.nconv); returns
        (CG iterations, true |b - A x|^2/|b|^2, reliable updates) per system"""
        n = len(x_ids)
        nev = _deflate_args(basis, nev, n)
        sloppy = _batch_sloppy(sloppy)
        rq = [float(r2req)] * n if np.isscalar(r2req) else [float(v) for v in r2req]
        its, fin, nup = (C.c_int * n)(), (C.c_double * n)(), (C.c_int * n)()
        check(lib().qexhip_dev_solve_xx_batch_deflated(self._h, int(basis.id), nev, n, (C.c_int * n)(*[int(v) for v in x_ids]),
                                                       (C.c_int * n)(*[int(v) for v in b_ids]), (C.c_double * n)(*[float(v) for v in masses]),
                                                       (C.c_double * n)(*rq), int(maxits), 1 if par_even else 0, sloppy, its, fin, nup))
        return list(its), list(fin), list(nup)

    def dev_op_xx_sloppy(self, r_id, x_id, m2, par_even=True):
        """r[par] = 4 m2 x - (2D)(2D) x with the sloppy solve's fp32 links and sweep (x rounded to fp32, the result back to fp64)"""
        check(lib().qexhip_dev_op_xx_sloppy(self._h, int(r_id), int(x_id), float(m2), 1 if par_even else 0))

    def links_info_f32(self):
        """(format, max deviation) of the fp32 link copy of the sloppy solves: 0 = 18 reals, 1 = rows 0,1 + sign"""
        f, dev = C.c_int(0), C.c_double(0)
        check(lib().qexhip_stag_links_info_f32(self._h, C.byref(f), C.byref(dev)))
        return f.value, dev.value

    def dev_op_xx_half(self, r_id, x_id, m2, par_even=True):
        """r[par] = 4 m2 x - (2D)(2D) x with the 16-bit links, vectors and sweep of SloppyHalf under option "half" = 1 (x rounded to
        the 16-bit format, the intermediate and the result stored in it, the result back to fp64).  On a t-sharded context: collective
        (the faces are exchanged in the 16-bit format), and the slab of the one-rank operator's result, bit for bit"""
        check(lib().qexhip_dev_op_xx_half(self._h, int(r_id), int(x_id), float(m2), 1 if par_even else 0))

    def links_info_half(self):
        """(format, s_fat, s_long, max deviation) of the 16-bit link copy: format 0 = 18 reals scaled by the largest |entry| of the
        link kind (s_fat, s_long), 1 = rows 0,1 + the fp32 copy's sign masks (scale 1).  On a t-sharded context every rank gets the
        values of the whole lattice, and the call is collective where the copy has to be rebuilt"""
        f, sf, sl, dev = C.c_int(0), C.c_double(0), C.c_double(0), C.c_double(0)
        check(lib().qexhip_stag_links_info_half(self._h, C.byref(f), C.byref(sf), C.byref(sl), C.byref(dev)))
        return f.value, sf.value, sl.value, dev.value

    def sloppy_last(self):
        """what the last single-system sloppy solve ran (qexhip_stag_sloppy_last): dict with precision (1 single, 2 16-bit storage),
        half_iters, f32_iters and fell_back (the 16-bit solve's stall guard handed over to fp32)"""
        v = [C.c_int(0) for _ in range(4)]
        check(lib().qexhip_stag_sloppy_last(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("precision", "half_iters", "f32_iters", "fell_back"), (x.value for x in v)))

    def dev_op_xx_half_batch(self, r_ids, x_ids, m2s, par_even=True):
        """the batched form of dev_op_xx_half (qexhip_dev_op_xx_half_batch): n <= 4 fields rounded to the 16-bit format, one batched
        operator with its own m2 per system (the links streamed once for all of them), the results back in fp64.  One rank without
        ghost zones; with set_option("batch_ranks", 1) on a t-sharded context too: collective (all systems' 16-bit faces in one
        exchange per sweep), every system's slab of the one-rank single-system operator's result, bit for bit"""
        self._op_xx_batch("qexhip_dev_op_xx_half_batch", r_ids, x_ids, m2s, par_even)

    def dev_op_xx_sloppy_batch(self, r_ids, x_ids, m2s, par_even=True):
        """the fp32 twin of dev_op_xx_half_batch (qexhip_dev_op_xx_sloppy_batch): n <= 4 fields rounded to fp32, one batched fp32
        operator with its own m2 per system, the results back in fp64; t-sharded contexts with set_option("batch_ranks", 1)"""
        self._op_xx_batch("qexhip_dev_op_xx_sloppy_batch", r_ids, x_ids, m2s, par_even)

    def _op_xx_batch(self, entry, r_ids, x_ids, m2s, par_even):
        n = len(x_ids)
        if len(r_ids) != n or len(m2s) != n:
            raise ValueError("%s: r_ids, x_ids and m2s differ in length" % entry[len("qexhip_"):])
        check(getattr(lib(), entry)(self._h, n, (C.c_int * max(n, 1))(*[int(v) for v in r_ids]),
                                    (C.c_int * max(n, 1))(*[int(v) for v in x_ids]),
                                    (C.c_double * max(n, 1))(*[float(v) for v in m2s]), 1 if par_even else 0))

    def sloppy_last_batch(self):
        """what the last batched sloppy call ran per system (qexhip_stag_sloppy_last_batch): a list of dicts as sloppy_last()'s"""
        n = C.c_int(0)
        v = [(C.c_int * 4)() for _ in range(4)]
        check(lib().qexhip_stag_sloppy_last_batch(self._h, 4, C.byref(n), *v))
        keys = ("precision", "half_iters", "f32_iters", "fell_back")
        return [dict(zip(keys, (a[j] for a in v))) for j in range(min(n.value, 4))]

    def release_workspace(self):
        check(lib().qexhip_release_workspace(self._h))

    def dev_zero(self, fid, subset="all"):
        check(lib().qexhip_dev_zero(self._h, int(fid), _SUBSET[subset]))

    def dev_solve_batch(self, x_ids, b_ids, masses, r2req, maxits=1000000, sloppy=None, deflate=None, nev=None):
        """n x Staggered.solve on resident fields (lock-step batches of four); returns (iterations, r2) per system.
        sloppy = 0, 1 or 2 (SloppyNone / SloppySingle / SloppyHalf) chooses the precision of the batched CG explicitly
        (qexhip_dev_solve_batch_sloppy; mixed precision on one rank, and on t-sharded contexts with
        set_option("batch_ranks", 1) on every rank) and returns (iterations, r2, reliable updates).
        deflate = an EigBasis: the inner solveEE / solveOO batches are deflated from it with its leading nev vectors (None:
        deflate.nconv; qexhip_dev_solve_batch_deflated); the return value is that of the same call without it."""
        n = len(x_ids)
        rq = [float(r2req)] * n if np.isscalar(r2req) else [float(v) for v in r2req]
        its, fin = (C.c_int * n)(), (C.c_double * n)()
        if deflate is not None or nev is not None:
            nev = _deflate_args(deflate, nev, None)
        if sloppy is not None or deflate is not None:
            sl = 0 if sloppy is None else _batch_sloppy(sloppy)
            ms = [float(v) for v in masses]
            xi, bi = [int(v) for v in x_ids], [int(v) for v in b_ids]
            nup = []
            for k0 in range(0, n, 4):           # the entry takes one lock-step batch of at most four
                k = min(4, n - k0)
                i4, f4, u4 = (C.c_int * k)(), (C.c_double * k)(), (C.c_int * k)()
                a = ((C.c_int * k)(*xi[k0:k0 + k]), (C.c_int * k)(*bi[k0:k0 + k]), (C.c_double * k)(*ms[k0:k0 + k]),
                     (C.c_double * k)(*rq[k0:k0 + k]), int(maxits), sl, i4, f4, u4)
                if deflate is not None:
                    check(lib().qexhip_dev_solve_batch_deflated(self._h, int(deflate.id), nev, k, *a))
                else:
                    check(lib().qexhip_dev_solve_batch_sloppy(self._h, k, *a))
                its[k0:k0 + k], fin[k0:k0 + k] = list(i4), list(f4)
                nup += list(u4)
            if sloppy is None:
                return list(its), list(fin)
            return list(its), list(fin), nup
        check(lib().qexhip_dev_solve_batch(self._h, n, (C.c_int * n)(*[int(v) for v in x_ids]), (C.c_int * n)(*[int(v) for v in b_ids]),
                                           (C.c_double * n)(*[float(v) for v in masses]), (C.c_double * n)(*rq), int(maxits), its, fin))
        return list(its), list(fin)

    def dev_norm2(self, x_id, subset="all"):
        out = C.c_double(0)
        check(lib().qexhip_dev_norm2(self._h, x_id, _SUBSET[subset], C.byref(out)))
        return out.value

    def dev_redot(self, x_id, y_id, subset="all"):
        out = C.c_double(0)
        check(lib().qexhip_dev_redot(self._h, x_id, y_id, _SUBSET[subset], C.byref(out)))
        return out.value

    def dev_dot(self, x_id, y_id, subset="all"):
        """dot(x, y) = sum x^+ y of resident fields (fieldET.nim:677-693), complex"""
        out = (C.c_double * 2)()
        check(lib().qexhip_dev_dot(self._h, x_id, y_id, _SUBSET[subset], out))
        return complex(out[0], out[1])

    def dev_D(self, r_id, x_id, m, sc=1.0):
        """r = m x + sc D x on resident fields (Staggered.D: sc = 1, Ddag: sc = -1)"""
        check(lib().qexhip_dev_D(self._h, r_id, x_id, float(m), float(sc)))

    def dev_meson_corners(self, x_ids, y_ids, t0=0):
        """stagLocalMesons (fpvaMeas.nim:33-61) summed over the pairs (x_ids[k], y_ids[k]), k < 4: (nt, 8) array, rank-global"""
        n = len(x_ids)
        if n != len(y_ids):
            raise ValueError("x_ids and y_ids differ in length")
        nt = self.lat[3] * self.rank_geom[3]
        out = np.zeros((nt, 8))
        check(lib().qexhip_dev_meson_corners(self._h, n, (C.c_int * max(n, 1))(*[int(v) for v in x_ids]),
                                             (C.c_int * max(n, 1))(*[int(v) for v in y_ids]), int(t0), _p(out)))
        return out

    def dev_sym_shift(self, r_id, x_id, mu):
        """symShift (fpvaMeas.nim:16-31) with the operator's one-hop links: r = U_mu x(+mu) + U_mu(-mu)^+ x(-mu), mu < 3"""
        check(lib().qexhip_dev_sym_shift(self._h, int(r_id), int(x_id), int(mu)))

    def dev_norm2slice(self, fid, dir):
        """norm2slice (sources.nim:10-18): |f|^2 summed over the slices of direction dir, rank-global"""
        n = self.lat[dir] * (self.rank_geom[3] if dir == 3 else 1) if 0 <= dir < 4 else 1     # (the library refuses any other dir)
        out = np.zeros(n)
        check(lib().qexhip_dev_norm2slice(self._h, int(fid), int(dir), _p(out)))
        return out

    # stochastic scalar trace (scalarTrace.nim; csrc/trace.hip): complex site fields, dilution, <a, b> accumulation, slice sums
    def cfield_new(self):
        """a resident complex site field (lo.Complex), zeroed; its ids are separate from the colour vectors'"""
        cid = C.c_int(0)
        check(lib().qexhip_cfield_new(self._h, C.byref(cid)))
        return cid.value

    def cfield_free(self, cid):
        check(lib().qexhip_cfield_free(self._h, int(cid)))

    def cfield_zero(self, cid):
        check(lib().qexhip_cfield_zero(self._h, int(cid)))

    def cfield_scale(self, cid, s):
        check(lib().qexhip_cfield_scale(self._h, int(cid), float(s)))

    def cfield_axpy(self, dst, a, src):
        """dst += a * src on every site, both components (dst != src)"""
        check(lib().qexhip_cfield_axpy(self._h, int(dst), float(a), int(src)))

    def cfield_download(self, cid):
        """(vol, 2) array of (re, im) in the site order of field_download"""
        out = np.zeros((self.vol, 2))
        check(lib().qexhip_cfield_download(self._h, int(cid), _p(out)))
        return out

    def dev_dilute(self, dst_ids, src_id, kind, idx, t, scale=1.0):
        """dst_k = scale * src on the sites of GLOBAL time t[k] in pattern idx[k] of kind 0 (EO: global parity) or 1 (CORNER:
        (x0&1) | (x1&1)<<1 | (x2&1)<<2), exact zeros elsewhere; up to four destinations in one launch"""
        n = len(dst_ids)
        if n != len(idx) or n != len(t):
            raise ValueError("dst_ids, idx and t differ in length")
        i = C.c_int * max(n, 1)
        check(lib().qexhip_dev_dilute(self._h, n, i(*[int(v) for v in dst_ids]), int(src_id), int(kind), i(*[int(v) for v in idx]),
                                      i(*[int(v) for v in t]), float(scale)))

    def dev_trace_accum(self, cid, a_ids, b_ids, coef=1.0):
        """trce(x) += coef * a_k(x).dot b_k(x) for up to four pairs, one after the other in ascending k"""
        n = len(a_ids)
        if n != len(b_ids):
            raise ValueError("a_ids and b_ids differ in length")
        i = C.c_int * max(n, 1)
        check(lib().qexhip_dev_trace_accum(self._h, int(cid), n, i(*[int(v) for v in a_ids]), i(*[int(v) for v in b_ids]), float(coef)))

    def dev_cfield_slices(self, cid):
        """(nt, 2) array: Re, Im of the sum of the cfield over every global time slice, rank-global"""
        out = np.zeros((self.lat[3] * self.rank_geom[3], 2))
        check(lib().qexhip_dev_cfield_slices(self._h, int(cid), _p(out)))
        return out

    # connected scalar correlator (conn4d.nim; csrc/conn.hip): point sources, translated |phi|^2 accumulation, staggered sign
    def dev_point_source(self, ids, pts, ic):
        """field ids[k] := 0, then 1 + 0i in colour ic[k] at the GLOBAL coordinate pts[k] = (x, y, z, t); up to four in one launch"""
        n = len(ids)
        if n != len(pts) or n != len(ic) or any(len(p) != 4 for p in pts):
            raise ValueError("ids, pts (four coordinates each) and ic differ in length")
        i = C.c_int * max(n, 1)
        check(lib().qexhip_dev_point_source(self._h, n, i(*[int(v) for v in ids]), (C.c_int * max(4 * n, 1))(*[int(v) for p in pts for v in p]),
                                            i(*[int(v) for v in ic])))

    def dev_conn_accum(self, cid, phis, pts, scal):
        """Re cfield(x) += scal * |phi_k(x (+) pts[k])|^2 for up to four propagators, one after the other in ascending k; (+) wraps
        over the GLOBAL extents, so the source point pts[k] lands on the origin"""
        n = len(phis)
        if n != len(pts) or any(len(p) != 4 for p in pts):
            raise ValueError("phis and pts (four coordinates each) differ in length")
        check(lib().qexhip_dev_conn_accum(self._h, int(cid), n, (C.c_int * max(n, 1))(*[int(v) for v in phis]),
                                          (C.c_int * max(4 * n, 1))(*[int(v) for p in pts for v in p]), float(scal)))

    def cfield_stag_sign(self, cid):
        """cfield(x) *= (-1)^(x0+x1+x2), in place"""
        check(lib().qexhip_cfield_stag_sign(self._h, int(cid)))

    # field algebra hooks (fieldET.nim:605-625,704-724)
    def norm2(self, x, subset="all"):
        out = C.c_double(0)
        check(lib().qexhip_norm2(self._h, _p(x), _SUBSET[subset], C.byref(out)))
        return out.value

    def redot(self, x, y, subset="all"):
        out = C.c_double(0)
        check(lib().qexhip_redot(self._h, _p(x), _p(y), _SUBSET[subset], C.byref(out)))
        return out.value

    def dot(self, x, y, subset="all"):
        """dot(x, y) = sum x^+ y (fieldET.nim:677-693), complex"""
        out = (C.c_double * 2)()
        check(lib().qexhip_dot(self._h, _p(x), _p(y), _SUBSET[subset], out))
        return complex(out[0], out[1])

    def axpy(self, a, x, y, subset="all"):
        check(lib().qexhip_axpy(self._h, a, _p(x), _p(y), _SUBSET[subset]))

    def xpay(self, x, a, y, subset="all"):
        check(lib().qexhip_xpay(self._h, _p(x), a, _p(y), _SUBSET[subset]))


class EigOpts(C.Structure):
    """qexhip_eig_opts: EigOpts of src/eigens/hisqev.nim (nev, nvecs, relerr, abserr, maxup) + the Chebyshev acceleration"""
    _fields_ = [("nev", C.c_int), ("nvecs", C.c_int), ("relerr", C.c_double), ("abserr", C.c_double), ("max_restarts", C.c_int),
                ("cheb_degree", C.c_int), ("cheb_lo", C.c_double), ("cheb_hi", C.c_double), ("seed", C.c_ulonglong)]


def eig_check_opts(**kw):
    """the option checks of Staggered.eigs alone (host only): the library's return code, 0 or QEXHIP_ERR_ARG (-1)"""
    o = EigOpts(**kw)
    return lib().qexhip_eig_check_opts(C.byref(o))


def symeig_host(a):
    """qexhip_symeig_host: (w ascending, z with z[:, i] the eigenvector of w[i]) of a real symmetric matrix; no device needed"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    n = a.shape[0] if a.ndim == 2 else 0
    if a.ndim != 2 or a.shape[1] != n:
        raise ValueError("symeig_host: a square matrix")
    w, z = np.zeros(n), np.zeros((n, n))
    pd = C.POINTER(C.c_double)
    check(lib().qexhip_symeig_host(a.ctypes.data_as(pd), n, w.ctypes.data_as(pd), z.ctypes.data_as(pd)))
    return w, np.ascontiguousarray(z.T)       # the library's z is column-major


class EigBasis:
    """A resident basis of nvecs half-volume vectors on the even sites (qexhip_eig_new).  Staggered.eigs fills `evals`, `resid`,
    `nconv` and `stats`; `vector(i)` downloads v_i as a full-volume host field (odd sites zero)."""

    def __init__(self, ctx, nvecs):
        self.ctx, self.nvecs = ctx, int(nvecs)
        bid = C.c_int(0)
        check(lib().qexhip_eig_new(ctx._h, self.nvecs, C.byref(bid)))
        self.id = bid.value
        self.evals, self.resid, self.nconv, self.stats = np.zeros(0), np.zeros(0), 0, {}

    def free(self):
        if self.id:
            check(lib().qexhip_eig_free(self.ctx._h, self.id))
            self.id = 0

    def get_vector(self, i, field_id):
        check(lib().qexhip_eig_get_vector(self.ctx._h, self.id, int(i), int(field_id)))

    def set_vector(self, i, field):
        """v_i := the even half of a resident field (id) or of a host array"""
        if isinstance(field, np.ndarray):
            fid = self.ctx.field_new(field)
            try:
                check(lib().qexhip_eig_set_vector(self.ctx._h, self.id, int(i), fid))
            finally:
                self.ctx.field_free(fid)
        else:
            check(lib().qexhip_eig_set_vector(self.ctx._h, self.id, int(i), int(field)))

    def vector(self, i):
        fid = self.ctx.field_new()
        try:
            self.get_vector(i, fid)
            return self.ctx.field_download(fid)
        finally:
            self.ctx.field_free(fid)

    def block_dot(self, i0, n, w_id):
        """[<v_j, w.even> for j in i0 .. i0+n-1] with w a resident field: complex array"""
        out = np.zeros(2 * n)
        check(lib().qexhip_eig_block_dot(self.ctx._h, self.id, int(i0), int(n), int(w_id), out.ctypes.data))
        return out[0::2] + 1j * out[1::2]

    def block_axpy(self, i0, coef, y_id):
        """y.even += sum_j coef[j] v_{i0+j} on the resident field y"""
        cf = np.asarray(coef, dtype=np.complex128)
        buf = np.ascontiguousarray(np.stack([cf.real, cf.imag], axis=-1))
        check(lib().qexhip_eig_block_axpy(self.ctx._h, self.id, int(i0), len(cf), buf.ctypes.data, int(y_id)))

    def block_dot_multi(self, i0, n, w_ids):
        """[[<v_j, w_k.even> for j in i0 .. i0+n-1] for k] in one pass over the basis: complex array (nrhs, n), each number bit for
        bit block_dot's for w_k alone"""
        k = len(w_ids)
        out = np.zeros((k, n, 2))
        check(lib().qexhip_eig_block_dot_multi(self.ctx._h, self.id, int(i0), int(n), k, (C.c_int * max(k, 1))(*[int(v) for v in w_ids]),
                                               out.ctypes.data))
        return out[..., 0] + 1j * out[..., 1]

    def block_axpy_multi(self, i0, coef, y_ids):
        """y_k.even += sum_j coef[k][j] v_{i0+j} for the distinct resident fields y_ids, one pass over the basis"""
        cf = np.atleast_2d(np.asarray(coef, dtype=np.complex128))
        k = len(y_ids)
        if cf.shape[0] != k:
            raise ValueError("block_axpy_multi: one row of coefficients per field")
        buf = np.ascontiguousarray(np.stack([cf.real, cf.imag], axis=-1))
        check(lib().qexhip_eig_block_axpy_multi(self.ctx._h, self.id, int(i0), cf.shape[1], k, buf.ctypes.data,
                                                (C.c_int * max(k, 1))(*[int(v) for v in y_ids])))

    def rotate(self, Q):
        """V[:, 0:k] <- V[:, 0:m] Q in place, Q real (m, k); vectors k .. m-1 are scratch afterwards"""
        Q = np.asarray(Q, dtype=np.float64)
        m, k = Q.shape
        qf = np.asfortranarray(Q)
        check(lib().qexhip_eig_rotate(self.ctx._h, self.id, m, k, qf.ctypes.data))

    # low-mode averaging of the scalar trace (include/qexhip.h "LOW-MODE AVERAGING"; scalar_trace.scalarTrace(lma=True))
    def block_norm2_accum(self, i0, wgt, cid):
        """cfield.even(c).re += sum_j wgt[j] sum_col |v_{i0+j}(c,col)|^2 in one pass over the len(wgt) vectors; bit for bit the chain
        get_vector(i0+j, f) + dev_trace_accum(cid, [f], [f], wgt[j]).  Imaginary part and odd sites are not touched."""
        w = np.ascontiguousarray(wgt, dtype=np.float64).reshape(-1)
        check(lib().qexhip_eig_block_norm2_accum(self.ctx._h, self.id, int(i0), len(w), w.ctypes.data, int(cid)))

    def lowmode_diag(self, nev, mass, cid):
        """cfield.re += L(x), the site diagonal of P (D+m)^-1 for the leading nev modes, on both parities:
        sum_i m/(m^2+lambda_i) |v_i(x)|^2 on the even and sum_i m/(m^2+lambda_i) |(D_oe v_i)(x)|^2 / lambda_i on the odd sites, with
        lambda_i the Rayleigh quotients.  Exact for exact eigenpairs; t-sharded: collective."""
        check(lib().qexhip_eig_lowmode_diag(self.ctx._h, self.id, int(nev), float(mass), int(cid)))

    def project_out(self, nev, ids):
        """phi_k <- (1 - P) phi_k in place on both parities for 1..4 distinct resident fields, P the orthogonal projector onto the
        leading nev modes and their odd partners D_oe v_i / sqrt(lambda_i); each field's result is bit for bit what it is alone"""
        n = len(ids)
        check(lib().qexhip_eig_project_out(self.ctx._h, self.id, int(nev), n, (C.c_int * max(n, 1))(*[int(v) for v in ids])))

    def rayleigh(self, n):
        ev = np.zeros(n)
        check(lib().qexhip_eig_evals(self.ctx._h, self.id, int(n), ev.ctypes.data))
        return ev


class Staggered:
    """Staggered[G,T] (stagD.nim:19-22): the links `g` carry BC and phases (rephase)."""

    def eigs(self, nev, nvecs=None, relerr=1e-4, abserr=1e-6, max_restarts=100, cheb_degree=0, cheb_lo=0.0, cheb_hi=0.0,
             seed=987654321, basis=None):
        """hisqev (src/eigens/hisqev.nim): the nev lowest eigenpairs of H = -D_eo D_oe on the even sites (eigenvalues = sv^2), by
        thick-restart Lanczos on T_p(H) (qexhip_stag_eigs).  Returns an EigBasis (a new one of nvecs vectors unless `basis` is given)
        with evals (ascending), resid (true residuals), nconv, stats."""
        nvecs = int(nvecs) if nvecs is not None else max(2 * int(nev), int(nev) + 8)
        o = EigOpts(int(nev), nvecs, float(relerr), float(abserr), int(max_restarts), int(cheb_degree), float(cheb_lo), float(cheb_hi), int(seed))
        check(lib().qexhip_eig_check_opts(C.byref(o)))
        B = basis if basis is not None else EigBasis(self.ctx, nvecs)
        ev, rs = np.zeros(nev), np.zeros(nev)
        nc, st = C.c_int(0), (C.c_long * 4)()
        try:
            check(lib().qexhip_stag_eigs(self.ctx._h, B.id, C.byref(o), C.byref(nc), ev.ctypes.data, rs.ctypes.data, st))
        except Exception:
            if basis is None:
                B.free()
            raise
        B.evals, B.resid, B.nconv = ev, rs, nc.value
        B.stats = dict(zip(("op_applications", "restarts", "lanczos_steps", "residual_checks"), [int(v) for v in st]))
        return B

    def __init__(self, ctx, g, g3=None, smear=None, bc="pppa"):
        """smear = None: g (, g3) are the final links.  smear = HisqCoefs(): the operator uses the
        HISQ fat + long links of g, built on the device.  smear = HypCoefs(...): it uses
        rephase(nHYP(g)) with boundary string `bc` ('a' = antiperiodic, as input_hmc.xml:44); with
        g = None the links come from the closure of a preceding HypCoefs.smearGetForce."""
        self.ctx = ctx
        self.g = g
        self.g3 = g3
        if smear is None:
            self.nlinks = 8 if g3 is not None else 4
            check(lib().qexhip_stag_set_links(ctx._h, _p(g), _p(g3)))
        elif isinstance(smear, HisqCoefs):
            self.nlinks = 8
            check(lib().qexhip_stag_set_links_hisq(ctx._h, _p(g) if g is not None else None))
        else:
            self.nlinks = 4
            ap = (C.c_int * 4)(*[1 if ch == "a" else 0 for ch in bc])
            check(lib().qexhip_stag_set_links_nhyp(ctx._h, _p(g) if g is not None else None, float(smear.alpha1), float(smear.alpha2),
                                                   float(smear.alpha3), ap, None))

    # r = m*x + D*x  /  r = m*x - D*x
    def links_info(self):
        """(links per site, format, max deviation) of the operator's links; format 0: 18 reals,
        1: rows 0,1 + sign bit (SU(3) x sign), 2: rows 0,1 + determinant (U(3))"""
        n, cflag, dev = C.c_int(0), C.c_int(0), C.c_double(0)
        check(lib().qexhip_stag_links_info(self.ctx._h, C.byref(n), C.byref(cflag), C.byref(dev)))
        return n.value, cflag.value, dev.value

    def links_storage(self):
        """(bytes per link the sweep streams, links escaped by the last lossless encoding): 144 / 96 / 112 for formats 0 / 1 / 2,
        108 for the lossless residual format, 100 for its packed form and 92 for its orthogonal form (the 18-real operator bit for
        bit: links_info reports format 0)"""
        nb, ne = C.c_int(0), C.c_longlong(0)
        check(lib().qexhip_stag_links_storage(self.ctx._h, C.byref(nb), C.byref(ne)))
        return nb.value, ne.value

    def D(self, r, x, m):
        check(lib().qexhip_stag_D(self.ctx._h, _p(r), _p(x), float(m), 1.0))

    def symShift(self, r, x, mu):
        """symShift (fpvaMeas.nim:16-31): r = U_mu(x) x(x+mu) + U_mu(x-mu)^+ x(x-mu), mu in 0..2, with this operator's one-hop links
        (the rephased g of newStag(g); the smeared one-hop links of a HISQ or nHYP operator).  r, x: field ids or host arrays."""
        if isinstance(r, np.ndarray) or isinstance(x, np.ndarray):
            ctx = self.ctx
            fx, fr = ctx.field_new(x), ctx.field_new()
            try:
                ctx.dev_sym_shift(fr, fx, mu)
                r[...] = ctx.field_download(fr)
            finally:
                ctx.field_free(fx)
                ctx.field_free(fr)
        else:
            self.ctx.dev_sym_shift(r, x, mu)

    def Ddag(self, r, x, m):
        check(lib().qexhip_stag_D(self.ctx._h, _p(r), _p(x), float(m), -1.0))

    def peqDdag(self, r, x, m):
        """r += m*x - D*x  (stagD.nim:572-574)"""
        check(lib().qexhip_stag_D_acc(self.ctx._h, _p(r), _p(x), float(m), -1.0, 1.0))

    def stagDeriv(self, f, x):
        """stagDeriv(s, f, x) without the final rephase (stagD.nim:634-663): f[mu] +-= x (x) x(+mu)^+"""
        check(lib().qexhip_stag_outer(self.ctx._h, _p(f), _p(x), 1.0, -1.0, 1))

    def outer(self, f, psi, scale, accumulate):
        """f[mu][i][a,b] (:= | +=) scale * psi[i][a] * psi(i+mu)[b].adj  (staghmc_spv.nim:831-854)"""
        check(lib().qexhip_stag_outer(self.ctx._h, _p(f), _p(psi), float(scale), float(scale), 1 if accumulate else 0))

    def stagD(self, r, x, subset, m, sc=1.0, a=0.0):
        """stagD(s.se | s.so, r, s.g, x, m, sc, a) (stagD.nim:406-409): r[subset] = a*r + m*x + sc*D*x"""
        check(lib().qexhip_stag_stagD(self.ctx._h, _p(r), _p(x), _SUBSET[subset], float(m), float(sc), float(a)))

    def eoReduce(self, r, b, m):
        """r.even = (D^+ b).even  (stagD.nim:575-581); r.odd is kept"""
        check(lib().qexhip_stag_eo_reduce(self.ctx._h, _p(r), _p(b), float(m)))

    def eoReconstruct(self, r, b, m):
        check(lib().qexhip_stag_eo_reconstruct(self.ctx._h, _p(r), _p(b), float(m)))

    def stagD2(self, r, x, subset, a, b):
        """r[subset] = a*r + b*x + (2D)x  (stagD.nim:349-395)"""
        check(lib().qexhip_stag_dslash(self.ctx._h, _p(r), _p(x), _SUBSET[subset], float(a), float(b)))

    def stagD2ee(self, r, x, m2):
        check(lib().qexhip_stag_op_xx(self.ctx._h, _p(r), _p(x), float(m2), 1))

    def stagD2oo(self, r, x, m2):
        check(lib().qexhip_stag_op_xx(self.ctx._h, _p(r), _p(x), float(m2), 0))

    def _flops(self, its):
        # (s.g.len*4*72+60)*nEven*iterations  (stagSolve.nim:92)
        return float((self.nlinks * 4 * 72 + 60) * (self.ctx.vol // 2) * its)

    def _record(self, sp, its, r2, seconds, nup=0):
        """what one finished solve adds to its SolverParams (stagSolve.nim:88-94; nup: reliable updates of a mixed-precision solve)"""
        sp.calls += 1
        sp.iterations += its
        sp.iterationsMax = max(sp.iterationsMax, its)
        sp.seconds += seconds
        sp.flops += self._flops(its)
        sp.r2 = r2
        sp.reliableUpdates += nup

    def solveXX(self, r, x, m, sp, parEven=True, histcap=0, deflate=None, nev=None):
        """solveXX(s, r, x, m, sp0, parEven) (stagSolve.nim:57-132): r <- solution, x = rhs.
        deflate = an EigBasis (even sites only): the deflated solve of hisqev.nim:653-705 with its leading nev vectors (default: the
        pairs Staggered.eigs returned); sp.r2 is then the TRUE residual and no history is kept."""
        t0 = time.time()
        its, fin, nup = C.c_int(0), C.c_double(0), C.c_int(0)
        hist = np.zeros(max(histcap, 1))
        sloppy = int(getattr(sp, "sloppySolve", SloppyNone))
        if deflate is not None:
            if not parEven:
                raise ValueError("deflate= applies to the even sites (solveEE)")
            n = len(deflate.evals) if nev is None else int(nev)
            check(lib().qexhip_stag_solve_xx_deflated(self.ctx._h, deflate.id, n, _p(r), _p(x), float(m), float(sp.r2req), int(sp.maxits),
                                                      sloppy, C.byref(its), C.byref(fin)))
            histcap = 0
        elif sloppy != SloppyNone:
            # mixed precision (no residual history: the fp32 iterations' residuals are not the true ones)
            check(lib().qexhip_stag_solve_xx_sloppy(self.ctx._h, _p(r), _p(x), float(m), float(sp.r2req), int(sp.maxits),
                                                    1 if parEven else 0, sloppy, C.byref(its), C.byref(fin), C.byref(nup)))
            histcap = 0
        else:
            check(lib().qexhip_stag_solve_xx(self.ctx._h, _p(r), _p(x), float(m), float(sp.r2req), int(sp.maxits),
                                             1 if parEven else 0, C.byref(its), C.byref(fin), _p(hist), histcap))
        self._record(sp, its.value, fin.value, time.time() - t0, nup.value)
        sp.r2hist = hist[: min(histcap, its.value + 1)] if histcap else None
        if sp.verbosity > 1:
            print(("solveEE" if parEven else "solveOO") + "(HIP): " + sp.getStats())

    def solveEE(self, r, x, m, sp, histcap=0, deflate=None, nev=None):
        self.solveXX(r, x, m, sp, True, histcap, deflate=deflate, nev=nev)

    def solveOO(self, r, x, m, sp, histcap=0, deflate=None, nev=None):
        """deflate = an EigBasis (of the EVEN sites): the odd solve deflated from it, through the deflated batch with one system"""
        if deflate is None and nev is None:
            return self.solveXX(r, x, m, sp, False, histcap)
        t0 = time.time()
        its, fin, nup = self._batch("xx", [r], [x], [m], sp.r2req, sp.maxits, False, int(getattr(sp, "sloppySolve", SloppyNone)),
                                    deflate=deflate, nev=nev)
        self._record(sp, its[0], fin[0], time.time() - t0, nup[0])
        sp.r2hist = None
        if sp.verbosity > 1:
            print("solveOO(HIP): " + sp.getStats())

    def solve(self, x, b, m, sp, sloppy=None, deflate=None, nev=None):
        """Staggered.solve: x (array or list of arrays) <- D(m)^-1 b  (stagSolve.nim:224-294,347-446).
        deflate = an EigBasis (single mass, from x = 0): the inner solveEE calls deflate with its leading nev vectors.
        sloppy (mass lists only): None = fp64, and a SolverParams that asks for a sloppy solve is refused; 0, 1 or 2 = the precision
        of the inner multi-shift CG, chosen explicitly whatever sp says (qexhip_stag_solve_multi_sloppy)."""
        multi = isinstance(x, (list, tuple))
        if deflate is not None:
            if multi or sloppy is not None or sp.usePrevSoln:
                raise ValueError("deflate= applies to single-mass solves from x = 0 (precision from sp.sloppySolve)")
            t0 = time.time()
            its, fin = C.c_int(0), C.c_double(0)
            n = len(deflate.evals) if nev is None else int(nev)
            check(lib().qexhip_stag_solve_deflated(self.ctx._h, deflate.id, n, _p(x), _p(b), float(m), float(sp.r2req), int(sp.maxits),
                                                   int(getattr(sp, "sloppySolve", SloppyNone)), C.byref(its), C.byref(fin)))
            self._record(sp, its.value, fin.value, time.time() - t0)
            return
        if sloppy is not None:
            sloppy = _batch_sloppy(sloppy)
            if not multi:
                raise ValueError("sloppy= applies to mass lists; a single-mass solve takes its precision from sp.sloppySolve")
            t0 = time.time()
            its, fin, nup = C.c_int(0), C.c_double(0), C.c_int(0)
            ms = np.array([float(v) for v in m], dtype=np.float64)
            ptrs = _ptrs(x)
            check(lib().qexhip_stag_solve_multi_sloppy(self.ctx._h, ptrs, _p(b), _p(ms), len(x), float(sp.r2req), int(sp.maxits),
                                                       sloppy, C.byref(its), C.byref(fin), C.byref(nup)))
            self._record(sp, its.value, fin.value, time.time() - t0, nup.value)
            if sp.verbosity > 1:
                print("stagSolve(HIP): " + sp.getStats())
            return
        t0 = time.time()
        its, fin, nup = C.c_int(0), C.c_double(0), C.c_int(0)
        sloppy = int(getattr(sp, "sloppySolve", SloppyNone))
        if multi and sloppy != SloppyNone:
            raise ValueError("sloppySolve applies to single-mass solves only: a multi-shift solve runs in fp64 unless the "
                             "mixed-precision one is asked for with the keyword sloppy=1 (solve / solveXX_multi / dev_solve_xx_multi)")
        if sloppy != SloppyNone:
            check(lib().qexhip_stag_solve_sloppy(self.ctx._h, _p(x), _p(b), float(m), float(sp.r2req), int(sp.maxits),
                                                 1 if sp.usePrevSoln else 0, sloppy, C.byref(its), C.byref(fin), C.byref(nup)))
        elif isinstance(x, (list, tuple)):
            ms = np.array([float(v) for v in m], dtype=np.float64)
            ptrs = _ptrs(x)
            check(lib().qexhip_stag_solve_multi(self.ctx._h, ptrs, _p(b), _p(ms), len(x), float(sp.r2req),
                                                int(sp.maxits), C.byref(its), C.byref(fin)))
        else:
            check(lib().qexhip_stag_solve_prev(self.ctx._h, _p(x), _p(b), float(m), float(sp.r2req), int(sp.maxits),
                                               1 if sp.usePrevSoln else 0, C.byref(its), C.byref(fin)))
        self._record(sp, its.value, fin.value, time.time() - t0, nup.value)
        if sp.verbosity > 1:
            print("stagSolve(HIP): " + sp.getStats())

    def _batch(self, fn_name, xs, bs, ms, r2req, maxits, parEven=None, sloppy=None, deflate=None, nev=None):
        if sloppy is not None:
            sloppy = _batch_sloppy(sloppy)
        n = len(xs)
        if not (1 <= n <= 4 and len(bs) == n and len(ms) == n):
            raise ValueError("batch solve: 1..4 systems, one source and one mass each")
        if deflate is not None or nev is not None:
            nev = _deflate_args(deflate, nev, n)
        rq = [float(r2req)] * n if np.isscalar(r2req) else [float(v) for v in r2req]
        xp = _ptrs(xs)
        bp = _ptrs(bs)
        mv, rv = (C.c_double * n)(*[float(v) for v in ms]), (C.c_double * n)(*rq)
        its, fin = (C.c_int * n)(), (C.c_double * n)()
        if deflate is not None:
            nup = (C.c_int * n)()
            sl = 0 if sloppy is None else sloppy
            if parEven is None:
                check(lib().qexhip_stag_solve_batch_deflated(self.ctx._h, int(deflate.id), nev, n, xp, bp, mv, rv, int(maxits), sl, its, fin, nup))
            else:
                check(lib().qexhip_stag_solve_xx_batch_deflated(self.ctx._h, int(deflate.id), nev, n, xp, bp, mv, rv, int(maxits),
                                                                1 if parEven else 0, sl, its, fin, nup))
            if sloppy is None:
                return list(its), list(fin)
            return list(its), list(fin), list(nup)
        if sloppy is not None:
            nup = (C.c_int * n)()
            if parEven is None:
                check(lib().qexhip_stag_solve_batch_sloppy(self.ctx._h, n, xp, bp, mv, rv, int(maxits), sloppy, its, fin, nup))
            else:
                check(lib().qexhip_stag_solve_xx_batch_sloppy(self.ctx._h, n, xp, bp, mv, rv, int(maxits), 1 if parEven else 0,
                                                              sloppy, its, fin, nup))
            return list(its), list(fin), list(nup)
        if parEven is None:
            check(lib().qexhip_stag_solve_batch(self.ctx._h, n, xp, bp, mv, rv, int(maxits), its, fin))
        else:
            check(lib().qexhip_stag_solve_xx_batch(self.ctx._h, n, xp, bp, mv, rv, int(maxits), 1 if parEven else 0, its, fin))
        return list(its), list(fin)

    def solve_batch(self, xs, bs, ms, sps, sloppy=None, deflate=None, nev=None):
        """n (<= 4) x Staggered.solve on these links in lock-step: the links are streamed once per sweep for
        all systems.  sps: one SolverParams (shared r2req / maxits) or one per system; each gets the
        statistics of its own system, exactly as n calls of solve would record them.
        sloppy: None = fp64, and a SolverParams that asks for a sloppy solve is refused; 0, 1 or 2 (SloppyNone / SloppySingle /
        SloppyHalf) = the precision of the batched CG, chosen explicitly whatever sps say (mixed precision: one rank, or t-sharded with option "batch_ranks" = 1; every
        system comes out bit for bit as its own sloppy solve does; sp.reliableUpdates gets each system's updates).
        deflate = an EigBasis: the inner solveEE / solveOO batches are deflated from it (leading nev vectors; None: deflate.nconv)."""
        sl = [sps] * len(xs) if isinstance(sps, SolverParams) else list(sps)
        if sloppy is not None:
            sloppy = _batch_sloppy(sloppy)
        elif any(int(getattr(sp, "sloppySolve", SloppyNone)) != SloppyNone for sp in sl):
            raise ValueError("sloppySolve applies to single-system solves only: a lock-step batch runs in fp64 unless the "
                             "mixed-precision batch is asked for with the keyword sloppy=1 (solve_batch / solveXX_batch / "
                             "dev_solve_batch)")
        t0 = time.time()
        nup = [0] * len(xs)
        if sloppy is None:
            its, fin = self._batch("solve", xs, bs, ms, [sp.r2req for sp in sl], min(sp.maxits for sp in sl), deflate=deflate, nev=nev)
        else:
            its, fin, nup = self._batch("solve", xs, bs, ms, [sp.r2req for sp in sl], min(sp.maxits for sp in sl), sloppy=sloppy,
                                        deflate=deflate, nev=nev)
        dt = (time.time() - t0) / len(xs)
        for sp, i, f, u in zip(sl, its, fin, nup):
            self._record(sp, i, f, dt, u)
        return its

    def solveXX_batch(self, xs, bs, ms, r2req, maxits, parEven=True, sloppy=None, deflate=None, nev=None):
        """n (<= 4) x solveEE / solveOO in lock-step; returns (iterations, r2/b2) per system.  sloppy = 0, 1 or 2 chooses the
        precision explicitly (as in solve_batch) and returns (fp32 iterations, true r2/b2, reliable updates) per system.
        deflate = an EigBasis of the even sites: BOTH parities are deflated from it with its leading nev vectors (None:
        deflate.nconv); r2/b2 is then the true residual."""
        return self._batch("xx", xs, bs, ms, r2req, maxits, parEven, sloppy, deflate=deflate, nev=nev)

    def solveXX_multi(self, xs, b, shifts, sp, parEven=True, histcap=0, sloppy=None):
        """Staggered.solveXX(xs, b, ms, sp, subset) (stagSolve.nim:296-345): shifts[0] = base mass.
        sloppy: None = fp64, and a SolverParams that asks for a sloppy solve is refused; 0, 1 or 2 = the mixed-precision multi-shift
        solve (fp32 iterations with reliable updates on the base shift, then every shift refined on its true residual), chosen
        explicitly whatever sp says.  It returns the true |b - A_k x_k|^2/|b|^2 per shift (-1 each for sloppy=0, where the fp64
        solver does not compute them, and sp.r2 is left unchanged as by the fp64 call); sp.iterations gets the fp32 iterations of phase 1, sp.reliableUpdates its updates,
        sp.refineIterations the refinement iterations per shift, sp.r2 the largest per-shift residual.  No residual history."""
        if sloppy is not None:
            sloppy = _batch_sloppy(sloppy)
            if histcap > 0:
                raise ValueError("sloppy= with histcap > 0: the mixed-precision multi-shift solve keeps no residual history")
            n = len(xs)
            its, nup = C.c_int(0), C.c_int(0)
            fin, ref = (C.c_double * n)(), (C.c_int * n)()
            sh = np.array([float(v) for v in shifts], dtype=np.float64)
            ptrs = _ptrs(xs)
            check(lib().qexhip_stag_solve_xx_multi_sloppy(self.ctx._h, ptrs, _p(b), _p(sh), n, float(sp.r2req), int(sp.maxits),
                                                          1 if parEven else 0, sloppy, C.byref(its), fin, C.byref(nup), ref))
            sp.iterations += its.value
            sp.reliableUpdates += nup.value
            sp.refineIterations = list(ref)
            if sloppy:
                sp.r2 = max(fin)
            sp.r2hist = None
            return list(fin)
        if int(getattr(sp, "sloppySolve", SloppyNone)) != SloppyNone:
            raise ValueError("sloppySolve applies to single-mass solves only: a multi-shift solve runs in fp64 unless the "
                             "mixed-precision one is asked for with the keyword sloppy=1 (solve / solveXX_multi / dev_solve_xx_multi)")
        its = C.c_int(0)
        sh = np.array([float(v) for v in shifts], dtype=np.float64)
        hist = np.zeros(max(histcap, 1))
        ptrs = _ptrs(xs)
        check(lib().qexhip_stag_solve_xx_multi(self.ctx._h, ptrs, _p(b), _p(sh), len(xs), float(sp.r2req),
                                               int(sp.maxits), 1 if parEven else 0, C.byref(its), _p(hist), histcap))
        sp.iterations += its.value
        sp.r2hist = hist[: min(histcap, its.value + 1)] if histcap else None

    def rationalXX(self, out, b, mass, rat, sp, parEven=True, histcap=0):
        """out[par] = r(M^+M) b[par] for host arrays; rat: a qex_amd.rational.Rational or (f0, alpha, beta).  One accumulating
        multi-shift solve in fp64 (qexhip_stag_rational_xx); sp.iterations / sp.r2hist as solveXX_multi"""
        f0, alpha, beta = (rat.f0, rat.alpha, rat.beta) if hasattr(rat, "alpha") else rat
        al = np.array([float(v) for v in alpha], dtype=np.float64)
        be = np.array([float(v) for v in beta], dtype=np.float64)
        if al.shape != be.shape:
            raise ValueError("rationalXX: %d residues, %d poles" % (al.size, be.size))
        if int(getattr(sp, "sloppySolve", SloppyNone)) != SloppyNone:
            raise ValueError("rationalXX runs in fp64: the mixed-precision multi-shift solve refines every shift on its own solution "
                             "and cannot accumulate")
        its = C.c_int(0)
        hist = np.zeros(max(histcap, 1))
        check(lib().qexhip_stag_rational_xx(self.ctx._h, _p(out), _p(b), float(mass), float(f0), int(al.size), (C.c_double * al.size)(*al), (C.c_double * be.size)(*be),
                                            float(sp.r2req), int(sp.maxits), 1 if parEven else 0, C.byref(its), _p(hist), histcap))
        sp.iterations += its.value
        sp.r2hist = hist[: min(histcap, its.value + 1)] if histcap else None


def _deflate_args(deflate, nev, n):
    """the keywords deflate= / nev= of the batched solves, checked before any library call; returns nev (None -> deflate.nconv)"""
    if not isinstance(deflate, EigBasis):
        raise ValueError("deflate = %r: an EigBasis (Staggered.eigs); nev= needs deflate=" % (deflate,))
    if n is not None and not 1 <= n <= 4:
        raise ValueError("deflated batch: 1..4 systems (n = %d)" % n)
    nev = int(deflate.nconv) if nev is None else nev
    if isinstance(nev, bool) or not isinstance(nev, (int, np.integer)) or not 0 <= int(nev) <= deflate.nvecs:
        raise ValueError("nev = %r: 0 .. %d (the vectors of the basis)" % (nev, deflate.nvecs))
    return int(nev)


def _batch_sloppy(sloppy):
    """the explicit precision of a lock-step batch: 0, 1 or 2, checked before any library call"""
    if isinstance(sloppy, bool) or not isinstance(sloppy, (int, np.integer)) or not 0 <= int(sloppy) <= 2:
        raise ValueError("sloppy = %r: None (fp64, the default), 0 (SloppyNone), 1 (SloppySingle) or 2 (SloppyHalf, runs single)" % (sloppy,))
    return int(sloppy)


def newStag(ctx, g):
    return Staggered(ctx, g)


def newStag3(ctx, g, g3):
    return Staggered(ctx, g, g3)


def _link_lossless_host(entry, links, out_shape):
    a = np.asarray(links)
    if np.iscomplexobj(a):
        a = np.stack([a.real, a.imag], axis=-1)
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 18)
    n = a.shape[0]
    esc = np.zeros(n, dtype=np.uint8)
    out = np.zeros((n,) + out_shape, dtype=np.float64)
    check(getattr(lib(), entry)(a.ctypes.data, n, esc.ctypes.data, out.ctypes.data))
    return esc.astype(bool), out


def link_residual_host(links):
    """The lossless link format's encoder + decoder on the host (no device needed).  links: complex or (..., 3, 3, 2) real array
    of 3x3 matrices.  Returns (escaped: bool per link, row2: the decoded row 2 of every link, shape (n, 3, 2))."""
    return _link_lossless_host("qexhip_link_residual_host", links, (3, 2))


def link_packed_host(links):
    """The packed lossless link format's encoder + decoder on the host (no device needed).  links as for link_residual_host.
    Returns (escaped: bool per link, decoded: every link as decoded, shape (n, 3, 3, 2))."""
    return _link_lossless_host("qexhip_link_packed_host", links, (3, 3, 2))


def link_ortho_host(links):
    """The orthogonal lossless link format's encoder + decoder on the host (no device needed).  links as for link_residual_host.
    Returns (escaped: bool per link, decoded: every link as decoded, shape (n, 3, 3, 2))."""
    return _link_lossless_host("qexhip_link_ortho_host", links, (3, 3, 2))


def half_pack_host(v):
    """The 16-bit vector format of the SloppyHalf solves on the host (no device needed).  v: (..., 3, 2) real or (..., 3) complex
    sites.  Returns (q: int16 (n, 6), norm: float32 (n,)): norm = the site's largest |component|, q = rint(v 32767 / norm)."""
    a = np.asarray(v)
    if np.iscomplexobj(a):
        a = np.stack([a.real, a.imag], axis=-1)
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 6)
    n = a.shape[0]
    q = np.zeros((n, 6), dtype=np.int16)
    norm = np.zeros(n, dtype=np.float32)
    check(lib().qexhip_half_pack_host(a.ctypes.data_as(C.POINTER(C.c_double)), n, q.ctypes.data_as(C.POINTER(C.c_int16)),
                                      norm.ctypes.data_as(C.POINTER(C.c_float))))
    return q, norm


def half_unpack_host(q, norm):
    """the sites (n, 3, 2) that half_pack_host's (q, norm) stand for: q norm / 32767"""
    q = np.ascontiguousarray(q, dtype=np.int16).reshape(-1, 6)
    norm = np.ascontiguousarray(norm, dtype=np.float32).reshape(-1)
    if norm.shape[0] != q.shape[0]:
        raise ValueError("half_unpack_host: one norm per site")
    v = np.zeros((q.shape[0], 3, 2), dtype=np.float64)
    check(lib().qexhip_half_unpack_host(q.ctypes.data_as(C.POINTER(C.c_int16)), norm.ctypes.data_as(C.POINTER(C.c_float)), q.shape[0],
                                        v.ctypes.data_as(C.POINTER(C.c_double))))
    return v


# ---- gauge observables / Wilson flow (src/gauge/gaugeUtils.nim:213-282, src/gauge/wflow.nim:21-67) ----
def plaq(ctx, g=None):
    if g is not None:
        check(lib().qexhip_gauge_set(ctx._h, _p(g)))
    out = np.zeros(6)
    check(lib().qexhip_plaq(ctx._h, _p(out)))
    return out


_FLOW_KIND = {"Wilson": 0, "rect": 0, "adj": 1}


def gaugeForce(ctx, g, cplaq=1.0, rect=0.0, adjplaq=0.0):
    """gc.gaugeForce(g, f) (gaugeAction.nim:334-350) / gc.forceA(g, f) (:742-747) with
    gc = GaugeActionCoeffs(plaq, rect | adjplaq)."""
    if rect != 0.0 and adjplaq != 0.0:
        raise ValueError("rect and adjplaq are separate code paths in QEX (gaugeForce vs forceA)")
    check(lib().qexhip_gauge_set(ctx._h, _p(g)))
    f = np.zeros_like(g)
    kind = 1 if adjplaq != 0.0 else 0
    check(lib().qexhip_gauge_force_general(ctx._h, _p(f), float(cplaq), float(adjplaq if kind else rect), kind))
    return f


def flowEQ(ctx, loop=1, g=None):
    """[E_s, E_t, Q] of the resident (or given) gauge field: g.fmunu(loop) -> densityE, topoQ
    (gaugeUtils.nim:1162-1271; `EQ` of src/flow/gauge_flow.nim:360-379)."""
    if g is not None:
        check(lib().qexhip_gauge_set(ctx._h, _p(g)))
    out = np.zeros(3)
    check(lib().qexhip_flow_EQ(ctx._h, int(loop), _p(out)))
    return out


def flowMeasure(ctx, g=None):
    """(plaq[6], [E_s, E_t, Q]) of the resident (or given) field in one pass: what the measure block of a flow loop prints
    after every step (src/flow/gauge_flow.nim:139-156,360-379)"""
    if g is not None:
        check(lib().qexhip_gauge_set(ctx._h, _p(g)))
    pl, eq = np.zeros(6), np.zeros(3)
    check(lib().qexhip_flow_measure(ctx._h, _p(pl), _p(eq)))
    return pl, eq


def gaugeAction(ctx, g=None, plaq=1.0, rect=0.0, adjplaq=0.0):
    """gc.gaugeAction1(g) / gc.actionA(g) (gaugeAction.nim:61-142,614-681) of g (or of the resident field)"""
    if g is not None:
        check(lib().qexhip_gauge_set(ctx._h, _p(g)))
    out = C.c_double(0)
    check(lib().qexhip_gauge_action(ctx._h, float(plaq), float(rect), float(adjplaq), C.byref(out)))
    return out.value


def gaugeUpdate(ctx, g, p, t):
    """mdt: g := exp(t p) g in place (staghmc_sh.nim:429-435)"""
    check(lib().qexhip_gauge_set(ctx._h, _p(g)))
    check(lib().qexhip_gauge_update(ctx._h, _p(p), float(t)))
    check(lib().qexhip_gauge_get(ctx._h, _p(g)))


class ResidentMD:
    """mdt / mdv / the force-gradient shifts of QEX's HMC drivers (staghmc_sh.nim:429-640) on links and momenta that
    stay on the device between the updates (qexhip_md_*).  Forces are left on the device by `gauge_force()` (source 0)
    and by the nHYP closure called with f = None (source 1: `sf.gforce(None, ...)`, `sf.fforce_solve(None, ...)` of
    `HypCoefs.smearGetForce(ctx, None)`, which smears the resident links)."""

    GAUGE, NHYP = 0, 1

    def __init__(self, ctx):
        self.ctx = ctx

    def begin(self, g, p):
        """upload links (None: keep the resident ones) and momenta (None: keep the resident ones, e.g. RngField.dev_momenta)"""
        check(lib().qexhip_md_begin(self.ctx._h, _p(g), _p(p)))

    def end(self, g=None, p=None):
        check(lib().qexhip_md_end(self.ctx._h, _p(g), _p(p)))

    def momentum_norm2(self):
        out = C.c_double(0)
        check(lib().qexhip_md_momentum_norm2(self.ctx._h, C.byref(out)))
        return out.value

    def update_links(self, t):
        """mdt: U <- exp(t p) U"""
        check(lib().qexhip_md_update_links(self.ctx._h, float(t)))

    def gauge_force(self, plaq=1.0, rect=0.0, adjplaq=0.0):
        check(lib().qexhip_md_gauge_force(self.ctx._h, float(plaq), float(rect), float(adjplaq)))

    def kick(self, source, t):
        """mdv: p += t f"""
        check(lib().qexhip_md_kick(self.ctx._h, int(source), float(t)))

    def shift_links(self, source, t):
        """fgv / fgvf: U <- exp(t f) U"""
        check(lib().qexhip_md_shift_links(self.ctx._h, int(source), float(t)))

    def save_links(self):
        check(lib().qexhip_md_save_links(self.ctx._h))

    def restore_links(self):
        check(lib().qexhip_md_restore_links(self.ctx._h))

    def reunit_links(self):
        """g.projectSU on the resident links (qexhip_gauge_reunit)"""
        check(lib().qexhip_gauge_reunit(self.ctx._h))

    # ---- HISQ molecular dynamics (src/examples/hisqhmc.nim) on the resident fields: qexhip_md_hisq_* ----
    def hisq_prepare(self, antiperiodic=None, phases=None, set_links=True):
        """smearRephase (hisqhmc.nim:405-414) on the resident thin links, which stay as they are: the HISQ closure is built from a
        phased copy on the device (defaults: t antiperiodic, QEX's staggered phases); set_links also hands su, sul to the operator"""
        ap = (C.c_int * 4)(*[int(bool(v)) for v in antiperiodic]) if antiperiodic is not None else None
        ph = (C.c_int * 4)(*[int(v) for v in phases]) if phases is not None else None
        check(lib().qexhip_md_hisq_prepare(self.ctx._h, ap, ph, 1 if set_links else 0))

    def hisq_fforce(self, psi_ids, scale, t):
        """fermionForce (hisqhmc.nim:496-539) for the resident vectors psi_ids, left on the device (hisq_force()), and p += t f"""
        n = len(psi_ids)
        check(lib().qexhip_md_hisq_fforce(self.ctx._h, n, (C.c_int * n)(*[int(v) for v in psi_ids]),
                                          (C.c_double * n)(*[float(v) for v in scale]), float(t)))

    def hisq_fforce_solve(self, phi_ids, mass, scale, r2req, maxits, t):
        """the same with psi_k = D(mass_k)^-1 phi_k solved first on the operator's current links (lock-step batches of four);
        returns the iteration counts"""
        n = len(phi_ids)
        rq = [float(r2req)] * n if np.isscalar(r2req) else [float(v) for v in r2req]
        its = (C.c_int * n)()
        check(lib().qexhip_md_hisq_fforce_solve(self.ctx._h, n, (C.c_int * n)(*[int(v) for v in phi_ids]),
                                                (C.c_double * n)(*[float(v) for v in mass]), (C.c_double * n)(*[float(v) for v in scale]),
                                                (C.c_double * n)(*rq), int(maxits), float(t), its))
        return list(its)

    def hisq_fforce_rational(self, phi_id, mass, alpha, beta, r2req, maxits, t, sloppy=0):
        """the force of 1/2 Re<phi, r(M^+M) phi>_even, r(x) = f0 + sum_k alpha_k / (x + beta_k): every pole's vector from ONE
        multi-shift solve on phi.even, weights alpha_k / sqrt(mass^2 + beta_k), and p += t f; returns the iterations"""
        n = len(alpha)
        if len(beta) != n:
            raise ValueError("hisq_fforce_rational: %d residues, %d poles" % (n, len(beta)))
        its = C.c_int(0)
        check(lib().qexhip_md_hisq_fforce_rational(self.ctx._h, int(phi_id), float(mass), n, (C.c_double * n)(*[float(v) for v in alpha]),
                                                   (C.c_double * n)(*[float(v) for v in beta]), float(r2req), int(maxits), int(sloppy),
                                                   float(t), C.byref(its)))
        return its.value

    def hisq_force(self):
        """the last force of hisq_fforce / hisq_fforce_solve / hisq_fforce_rational, [vol][4][3][3][2]"""
        f = np.zeros((self.ctx.vol, 4, 3, 3, 2))
        check(lib().qexhip_md_hisq_force_get(self.ctx._h, _p(f)))
        return f


def reunit(ctx, g):
    """g.projectSU in place (gaugeUtils.nim:1333-1334)"""
    check(lib().qexhip_gauge_set(ctx._h, _p(g)))
    check(lib().qexhip_gauge_reunit(ctx._h))
    check(lib().qexhip_gauge_get(ctx._h, _p(g)))


def wline(ctx, path, g=None):
    """g.wline(path) (gaugeUtils.nim:1079-1112); path entries +-(mu+1)"""
    if g is not None:
        check(lib().qexhip_gauge_set(ctx._h, _p(g)))
    out = (C.c_double * 2)()
    arr = (C.c_int * len(path))(*[int(v) for v in path])
    check(lib().qexhip_wline(ctx._h, arr, len(path), out))
    return complex(out[0], out[1])


def s4_gauge(ctx, g=None):
    """g.s4_gauge() (stagg_pv_hmc/staghmc_spv_meas.nim:25-65): peo[dir][even/odd], a (4, 2) array, of g or of the resident field"""
    if g is not None:
        check(lib().qexhip_gauge_set(ctx._h, _p(g)))
    out = np.zeros(8)
    check(lib().qexhip_plaq_s4(ctx._h, _p(out)))
    return out.reshape(4, 2)


def ploops(ctx, g=None):
    """the four Polyakov loops [g.wline([mu+1] * L_mu) for mu in 0..3] (gauge_flow.nim:137-156 `meas_ploop`,
    staghmc_sh.nim:281-291 `ploop`) of g, or of the resident field, in one call"""
    if g is not None:
        check(lib().qexhip_gauge_set(ctx._h, _p(g)))
    out = np.zeros(8)
    check(lib().qexhip_polyakov_loops(ctx._h, _p(out)))
    return [complex(out[2 * d], out[2 * d + 1]) for d in range(4)]


def gaugeFlow(ctx, g, steps, eps, measure=None, flow_act="Wilson", plaq=1.0, rect=0.0, adjplaq=0.0):
    """g.gaugeFlow(steps, eps): measure (wflow.nim:21-67), or the fork's
    gc.gaugeFlow(flow_act, g, steps, eps): measure (src/flow/flow.nim:22-90) with
    gc = GaugeActionCoeffs(plaq, rect, adjplaq).  g is modified in place."""
    kind = _FLOW_KIND[flow_act]
    c2 = adjplaq if kind else rect
    check(lib().qexhip_gauge_set(ctx._h, _p(g)))
    if measure is None:
        check(lib().qexhip_wflow_general(ctx._h, int(steps), float(eps), float(plaq), float(c2), kind))
    else:
        for n in range(1, steps + 1):
            check(lib().qexhip_wflow_general(ctx._h, 1, float(eps), float(plaq), float(c2), kind))
            measure(n * eps)
    check(lib().qexhip_gauge_get(ctx._h, _p(g)))


def gaugeSet(ctx, g):
    """upload g as the context's resident gauge field (what plaq / gaugeFlow(..) with g given do first)"""
    check(lib().qexhip_gauge_set(ctx._h, _p(g)))


def gaugeFlowResident(ctx, steps, eps):
    """`steps` RK3 steps of g.gaugeFlow(steps, eps) (wflow.nim:21-67) on the resident field; nothing crosses PCIe"""
    check(lib().qexhip_wflow(ctx._h, int(steps), float(eps)))


# ---- link construction (src/gauge/fat7l.nim, src/physics/hisqLinks.nim, src/gauge/hypsmear.nim) ----
class HisqCoefs:
    """hisqLinks.nim:3-24: `var hc: HisqCoefs; hc.init(); hc.smear(g, fl, ll)`"""

    def init(self):
        return self

    def force(self, ctx, g, dsdsu, dsdsul):
        """smearGetForce(...)'s smearedForce(dsdu, dsdsu, dsdsul) (hisqsmear.nim:55-90); returns dsdu"""
        f = np.zeros_like(g)
        check(lib().qexhip_hisq_force(ctx._h, _p(g), _p(dsdsu), _p(dsdsul), _p(f)))
        return f

    def smear(self, ctx, g, fl, ll):
        check(lib().qexhip_hisq_smear(ctx._h, _p(g), _p(fl), _p(ll)))

    def smearGetForce(self, ctx, g, fl=None, ll=None):
        """hisqsmear.nim:55-90: smear g (into fl, ll if given) and return the closure smearedForce(dsdu, dsdsu, dsdsul);
        u, v, w, su, sul stay on the device until release().  Staggered(ctx, None, smear=HisqCoefs()) then builds the
        operator from the closure's links."""
        check(lib().qexhip_hisq_prepare(ctx._h, _p(g), _p(fl), _p(ll)))

        def smearedForce(dsdu, dsdsu, dsdsul):
            check(lib().qexhip_hisq_closure_force(ctx._h, _p(dsdsu), _p(dsdsul), _p(dsdu)))

        def fermionForce(f, psis, scales):
            """fermionForce (hisqhmc.nim:496-541) for the fields psis; the closure must hold the PHASED links"""
            n = len(psis)
            arr = _ptrs(psis)
            sc = (C.c_double * n)(*[float(v) for v in scales])
            check(lib().qexhip_hisq_fermion_force(ctx._h, _p(f), arr, sc, n))

        smearedForce.fermionForce = fermionForce
        smearedForce.release = lambda: check(lib().qexhip_hisq_release(ctx._h))
        return smearedForce


def fat7lDeriv(ctx, g, dfl, coef, dll=None, naik=0.0):
    """fat7lDeriv (fat7lderiv.nim): derivative through makeImpLinks(g, coef, naik) of the chains dfl (, dll)"""
    d = np.zeros_like(g)
    cf = (C.c_double * 5)(*[float(v) for v in coef])
    check(lib().qexhip_fat7_deriv(ctx._h, _p(g), _p(dfl), cf, _p(dll), float(naik), _p(d)))
    return d


class HypCoefs:
    """hypsmear.nim:15-18,260-275: `coef.smear(g, fl)` (forward smearing only)"""

    def __init__(self, alpha1=0.4, alpha2=0.5, alpha3=0.5):
        self.alpha1, self.alpha2, self.alpha3 = alpha1, alpha2, alpha3

    def smear(self, ctx, g, fl):
        check(lib().qexhip_nhyp_smear(ctx._h, _p(g), _p(fl), float(self.alpha1), float(self.alpha2), float(self.alpha3)))

    def smearGetForce(self, ctx, g, fl=None):
        """hypsmear.nim:49-247: smear g (into fl if given) and return the closure
        `smearedForce(f, chain)`; the intermediate fields stay on the device until the closure's
        `release()` (or the next smearGetForce on this context)."""
        check(lib().qexhip_nhyp_prepare(ctx._h, _p(g), float(self.alpha1), float(self.alpha2), float(self.alpha3), _p(fl)))

        def smearedForce(f, chain):
            check(lib().qexhip_nhyp_force(ctx._h, _p(f), _p(chain)))

        def gforce(f, plaq=1.0, rect=0.0, adjplaq=0.0):
            """gforce(act, g, sg, f, smear_force) (staghmc_spv.nim:217-228)"""
            check(lib().qexhip_nhyp_gauge_force(ctx._h, _p(f), float(plaq), float(rect), float(adjplaq)))

        def fforce(f, psis, scales, bc="aaaa"):
            """fforce + smeared_one_link_force (staghmc_spv.nim:716-865) for the fields psis"""
            n = len(psis)
            arr = _ptrs(psis)
            sc = (C.c_double * n)(*[float(v) for v in scales])
            ap = (C.c_int * 4)(*[1 if ch == "a" else 0 for ch in bc])
            check(lib().qexhip_nhyp_fermion_force(ctx._h, _p(f), arr, sc, n, ap, None))

        def fforce_solve(f, phis, masses, scales, r2req, maxits=1000000, bc="aaaa"):
            """the whole fforce incl. its solves (staghmc_sh.nim:387-427) on the operator's current links
            (build them from this closure: Staggered(ctx, None, smear=...)); returns the iteration counts"""
            n = len(phis)
            arr = _ptrs(phis)
            ms = (C.c_double * n)(*[float(v) for v in masses])
            sc = (C.c_double * n)(*[float(v) for v in scales])
            rq = (C.c_double * n)(*([float(r2req)] * n if np.isscalar(r2req) else [float(v) for v in r2req]))
            ap = (C.c_int * 4)(*[1 if ch == "a" else 0 for ch in bc])
            its = (C.c_int * n)()
            check(lib().qexhip_nhyp_fforce(ctx._h, _p(f), n, arr, ms, sc, rq, int(maxits), ap, None, its))
            return list(its)

        def fforce_solve_dev(f, phi_ids, masses, scales, r2req, maxits=1000000, bc="aaaa"):
            """fforce_solve with the pseudofermion fields resident (field ids of ctx)"""
            n = len(phi_ids)
            ids = (C.c_int * n)(*[int(v) for v in phi_ids])
            ms = (C.c_double * n)(*[float(v) for v in masses])
            sc = (C.c_double * n)(*[float(v) for v in scales])
            rq = (C.c_double * n)(*([float(r2req)] * n if np.isscalar(r2req) else [float(v) for v in r2req]))
            ap = (C.c_int * 4)(*[1 if ch == "a" else 0 for ch in bc])
            its = (C.c_int * n)()
            check(lib().qexhip_nhyp_fforce_dev(ctx._h, _p(f), n, ids, ms, sc, rq, int(maxits), ap, None, its))
            return list(its)

        smearedForce.gforce, smearedForce.fforce, smearedForce.fforce_solve = gforce, fforce, fforce_solve
        smearedForce.fforce_solve_dev = fforce_solve_dev
        smearedForce.release = lambda: check(lib().qexhip_nhyp_release(ctx._h))
        return smearedForce


def makeImpLinks(ctx, fl, g, coef, ll=None, naik=0.0):
    """makeImpLinks(fl, gf, coef, ll, gfLong, naik) with gfLong = gf (fat7l.nim:77-165);
    coef = (oneLink, threeStaple, fiveStaple, sevenStaple, lepage)."""
    cf = (C.c_double * 5)(*[float(v) for v in coef])
    check(lib().qexhip_fat7(ctx._h, _p(g), cf, _p(fl), _p(ll), float(naik)))
