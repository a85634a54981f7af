"""Per-site random number fields and the configuration generators on them: the host mirror of
newRNGField / gaussian / uniform / u1 (src/rng/distributionUtils.nim) and random / warm / randomTAH
(src/gauge/gaugeUtils.nim:1348-1446) over qexhip_rng_* (csrc/rng.hip).  Host only, no GPU needed."""
import ctypes as C

import numpy as np

from ._lib import check, lib

RngMilc6, MRG32k3a = 0, 1


class GlobalRng:
    """`var R: RngMilc6; R.seed(seed, 987654321)` (src/observables/conn4d.nim:63-65, staghmc_sh.nim:178-179): ONE RngMilc6 stream,
    not a field of them -- the global generator every rank advances alike.  Host only."""

    def __init__(self, seed, index=987654321):
        m = 0xFFFFFFFF
        s, self.r = int(seed) & m, []
        for _ in range(7):
            s = ((69607 + 8 * index) * s + 12345) & m
            self.r.append((s >> 8) & 0xFFFFFF)
        self.ic = ((69607 + 8 * index) * s + 12345) & m
        self.mult = (100005 + 8 * index) & m

    def uniform(self):
        """the next draw in [0, 1): a multiple of 2^-24, as the reference's float32 product gives it"""
        r = self.r
        t = (((r[5] >> 7) | (r[6] << 17)) ^ ((r[4] >> 1) | (r[5] << 23))) & 0xFFFFFF
        self.r = [t] + r[:6]
        self.ic = (self.ic * self.mult + 12345) & 0xFFFFFFFF
        return float(np.float32(t ^ ((self.ic >> 8) & 0xFFFFFF)) * np.float32(1.0 / 16777216.0))


class RngField:
    """lo.newRNGField(RngMilc6 | MRG32k3a, seed); for a t-sharded rank pass the global lattice and t_offset."""

    def __init__(self, lat, kind=RngMilc6, seed=987654321, glat=None, t_offset=0):
        self.lat = [int(v) for v in lat]
        self.vol = int(np.prod(self.lat))
        self._h = C.c_void_p()
        gl = (C.c_int * 4)(*[int(v) for v in glat]) if glat is not None else None
        check(lib().qexhip_rng_new(C.byref(self._h), int(kind), C.c_ulonglong(int(seed) & (2 ** 64 - 1)), (C.c_int * 4)(*self.lat),
                                   gl, int(t_offset)))

    def __del__(self):
        try:
            if self._h:
                lib().qexhip_rng_free(self._h)
        except Exception:
            pass

    def _new(self, *shape):
        return np.zeros((self.vol,) + shape)

    def uniform(self, ncomp):
        v = self._new(ncomp)
        check(lib().qexhip_rng_uniform(self._h, int(ncomp), v.ctypes.data_as(C.c_void_p)))
        return v

    def gaussian_vector(self):
        v = self._new(3, 2)
        check(lib().qexhip_rng_gaussian_vector(self._h, v.ctypes.data_as(C.c_void_p)))
        return v

    def u1_vector(self):
        v = self._new(3, 2)
        check(lib().qexhip_rng_u1_vector(self._h, v.ctypes.data_as(C.c_void_p)))
        return v

    def z4_vector(self):
        """v.z4 r (distributionUtils.nim:102-153): each colour component 1, i, -1 or -i by one uniform"""
        v = self._new(3, 2)
        check(lib().qexhip_rng_z4_vector(self._h, v.ctypes.data_as(C.c_void_p)))
        return v

    def z2_vector(self):
        """v.z2 r (distributionUtils.nim:154-180): each colour component 1 or -1 by one uniform"""
        v = self._new(3, 2)
        check(lib().qexhip_rng_z2_vector(self._h, v.ctypes.data_as(C.c_void_p)))
        return v

    def randomTAH(self):
        p = self._new(4, 3, 3, 2)
        check(lib().qexhip_rng_random_tah(self._h, p.ctypes.data_as(C.c_void_p)))
        return p

    def random(self):
        g = self._new(4, 3, 3, 2)
        check(lib().qexhip_rng_gauge_random(self._h, g.ctypes.data_as(C.c_void_p)))
        return g

    def warm(self, s):
        g = self._new(4, 3, 3, 2)
        check(lib().qexhip_rng_gauge_warm(self._h, float(s), g.ctypes.data_as(C.c_void_p)))
        return g

    # ---- the same draws written straight into HBM (RngMilc6 only; the field's state advances exactly as on the host) ----
    def dev_gaussian_vector(self, ctx, field_id):
        """v.gaussian r into the resident colour vector `field_id` of ctx"""
        check(lib().qexhip_rng_dev_gaussian_vector(ctx._h, self._h, int(field_id)))

    def dev_u1_vector(self, ctx, field_id):
        check(lib().qexhip_rng_dev_u1_vector(ctx._h, self._h, int(field_id)))

    def dev_z4_vector(self, ctx, field_id):
        """v.z4 r into a resident colour vector: the host fill's values and generator state bit for bit"""
        check(lib().qexhip_rng_dev_z4_vector(ctx._h, self._h, int(field_id)))

    def dev_z2_vector(self, ctx, field_id):
        check(lib().qexhip_rng_dev_z2_vector(ctx._h, self._h, int(field_id)))

    def dev_momenta(self, ctx):
        """p.randomTAH r into the resident MD momenta of ctx (qexhip_md_refresh_momenta)"""
        check(lib().qexhip_md_refresh_momenta(ctx._h, self._h))

    # ---- checkpoints: write_rng / read_rng of the fork (src/stagg_pv_hmc/staghmc_spv_rng.nim:135-182) ----
    def state(self):
        n = lib().qexhip_rng_state_words(self._h)
        w = np.zeros((self.vol, n), dtype=np.uint32)
        check(lib().qexhip_rng_get_state(self._h, w.ctypes.data_as(C.c_void_p)))
        return w

    def set_state(self, w):
        w = np.ascontiguousarray(w, dtype=np.uint32)
        if w.shape != (self.vol, lib().qexhip_rng_state_words(self._h)):
            raise ValueError("RNG state has the wrong shape")
        check(lib().qexhip_rng_set_state(self._h, w.ctypes.data_as(C.c_void_p)))

    def write(self, fn):
        """the generator field as one SciDAC record of typesize 36 (`writer.write(r.milc, recordMd)`)"""
        w = self.state()
        name = b"QDP_RngMilc6" if w.shape[1] == 9 else b"QDP_MRG32k3a"
        check(lib().qexhip_io_write_field(str(fn).encode(), (C.c_int * 4)(*self.lat), w.ctypes.data_as(C.c_void_p), 4 * w.shape[1], 4,
                                          name, b"F", 0, 1, None, b'<?xml version="1.0"?>\n<note>RNG field</note>\n'))

    def read(self, fn):
        w = np.zeros((self.vol, lib().qexhip_rng_state_words(self._h)), dtype=np.uint32)
        dt = C.create_string_buffer(64)
        check(lib().qexhip_io_read_field(str(fn).encode(), (C.c_int * 4)(*self.lat), w.ctypes.data_as(C.c_void_p), 4 * w.shape[1], 4, dt))
        self.set_state(w)
        return dt.value.decode()
