"""Straggler detection, MI355X-native (drop-in for nvidia_resiliency_ext.straggler).

Exports the reference's public names (reference straggler/__init__.py:16-18) plus
``StragglerReport`` (alias of ``Report``), ``ReportGenerator`` and ``KernelAttribution`` (what
``Detector.kernel_attribution`` returns), ``TailScore`` (what ``Detector.kernel_tail_score``
returns), ``IndividualTailScore`` (what ``Detector.kernel_individual_tail_score`` returns) and the
``histograms`` module (the fixed buckets of ``Detector.kernel_histograms``).
"""
from .reporting import (KernelAttribution, Report, ReportGenerator, StragglerId,  # noqa: F401
                        StragglerReport)
from .statistics import Statistic  # noqa: F401
from .straggler import (CallableId, Detector, IndividualTailScore,  # noqa: F401
                        KernelTailAttribution, TailScore)
from . import histograms, reporting  # noqa: F401
