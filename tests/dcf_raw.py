"""``pdc_dcf_scan`` and ``pdc_dcf_scan_dev`` called as C sees them, for what ``_cabi.dcf_scan`` cannot say: it takes
the sizes from its arrays and always passes its outputs, so a negative size, a NULL pointer or a size that disagrees
with the arrays reach the library only from here.  Shared by tests/test_dcf_host.py and tests/test_dcf_gpu.py."""
import numpy as np

from periodicity_amd import _cabi


def _address(v):
    """None, an address (a device pointer), or a numpy array's data."""
    return v if v is None or isinstance(v, int) else _cabi._ptr(v)


def _arguments(ta, a, tb, b, edges, na, nb, nlag, pairs, sums):
    na = ta.size if na is None else na
    nb = tb.size if nb is None else nb
    nlag = edges.size - 1 if nlag is None else nlag
    if pairs == "own":
        pairs = np.empty(max(nlag, 1), dtype=np.int64)
    if sums == "own":
        sums = np.empty(6 * max(nlag, 1))
    return na, nb, nlag, pairs, sums


def raw_scan(ta, a, tb, b, edges, na=None, nb=None, nlag=None, skip=0, chunk=0, pairs="own", sums="own"):
    """The host entry; sizes default to the arrays', outputs to arrays of this call.  Returns ``(pairs, sums)``."""
    na, nb, nlag, pairs, sums = _arguments(ta, a, tb, b, edges, na, nb, nlag, pairs, sums)
    _cabi.check(_cabi.lib().pdc_dcf_scan(_address(ta), _address(a), na, _address(tb), _address(b), nb, _address(edges),
                                         nlag, skip, chunk, _address(pairs), _address(sums), _cabi.default_device()))
    return pairs, sums


def raw_scan_dev(ta, a, tb, b, edges, na=None, nb=None, nlag=None, skip=0, chunk=0, pairs="own", sums="own"):
    """The device entry on the default stream.  Pointers are addresses of device buffers; numpy arrays are accepted only
    where the call is refused before any pointer is looked at."""
    na, nb, nlag, pairs, sums = _arguments(ta, a, tb, b, edges, na, nb, nlag, pairs, sums)
    _cabi.check(_cabi.lib().pdc_dcf_scan_dev(_cabi.default_device(), None, _address(ta), _address(a), na, _address(tb),
                                             _address(b), nb, _address(edges), nlag, skip, chunk, _address(pairs),
                                             _address(sums)))


def refusals(t, x, edges):
    """Keyword sets for ``raw_scan`` / ``raw_scan_dev`` that both refuse by their sizes and pointers alone."""
    good = dict(ta=t, a=x, tb=t, b=x, edges=edges)
    changes = (dict(na=-1), dict(nb=-1), dict(na=-1, nb=-1, skip=1), dict(na=1 << 31), dict(nb=(1 << 31) - 63),
               dict(nlag=0), dict(nlag=-1), dict(nlag=(1 << 22) + 1), dict(chunk=-1), dict(nb=t.size - 1, skip=1),
               dict(pairs=None), dict(sums=None), dict(pairs=None, sums=None), dict(edges=None, nlag=4),
               dict(ta=None, na=5), dict(a=None, na=5), dict(tb=None, nb=5), dict(b=None, nb=5))
    return [{**good, **change} for change in changes]
