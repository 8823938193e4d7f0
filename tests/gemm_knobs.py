"""The MMNAS_GEMM_* scheduling knobs for one test, shared by the GPU test modules' `gemm_tuning` fixtures."""
import os


def gemm_knobs():
    """Generator behind a fixture: yields set_knobs(**kw) -- MMNAS_GEMM_<KW> = value (None: unset) -- and restores the
    environment afterwards.  The library caches the knobs: it is told to re-read them after every change."""
    import mmnas_amd._lib as L
    saved = {}

    def set_knobs(**kw):
        for k, v in kw.items():
            name = 'MMNAS_GEMM_' + k.upper()
            saved.setdefault(name, os.environ.get(name))
            if v is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = str(v)
        L.lib().mmnas_gemm_reload_tuning()

    yield set_knobs
    for name, v in saved.items():
        if v is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = v
    L.lib().mmnas_gemm_reload_tuning()
