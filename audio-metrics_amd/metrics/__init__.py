"""Metric functions of the hot path, one module per reference module
(src/audio_metrics/metrics/{fad,kd,prdc,apa}.py; fad_stats.py, kad.py, kad_stats.py, kad_perm.py, mmd.py, neighbors.py, fidelity.py, pprecall.py, mauve.py, vendi.py, sinkhorn.py, sliced.py, classifier.py, fkea.py, fld.py, c2st.py, nn_test.py, dependence.py and retrieval.py are this build's own).  Submodules are kept importable by
name (``metrics.apa`` is the module, as in the reference), so nothing is re-exported here."""
from . import apa, c2st, classifier, dependence, fad, fad_stats, fidelity, fkea, fld, kad, kad_perm, kad_stats, kd, mauve, mmd, neighbors, nn_test, pprecall, prdc, retrieval, sinkhorn, sliced, vendi  # noqa: F401
