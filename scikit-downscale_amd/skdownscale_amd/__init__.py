"""skdownscale_amd -- MI355X-native engine for scikit-downscale's per-grid-cell hot path.

Public names mirror ``skdownscale.pointwise_models`` for the hot path only
(``skdownscale/pointwise_models/__init__.py:17-36`` of the reference).
"""
from .arrm import ArrmGridModel, PiecewiseLinearRegression, arrm_breakpoints
from .bcsd import BcsdGridModel, BcsdPrecipitation, BcsdTemperature
from .core import GridArray, GridDataset, PointWiseDownscaler
from .gard import AnalogGridModel, AnalogRegression, PureAnalog, PureRegression, RegressionGridModel
from .groupers import DAY_GROUPER, MONTH_GROUPER, PaddedDOYGrouper
from .grouping import GroupedGridModel, GroupedRegressor
from .regrid import InterpolatedGridArray, Regridder
from .remap import ConservativeRemapper, RemappedGridArray, cell_bounds
from .resample import GridResample, ResampledGridArray, time_bins
from .disagg import DisaggregatedGridArray, time_map
from .groupby import GridGroupBy, GroupAppliedGridArray, GroupReducedGridArray, group_labels
from .rolling import GridRolling, RolledGridArray
from .order_stats import TimeQuantileGridArray
from .spells import GridCondition, SpellGridArray
from .skill import GridComparison, SkillGridArray
from .distribution import DistributionGridArray
from .constructed import ConstructedAnalogs, ConstructedGridArray
from .localized import LocalizedAnalogs, LocalizedGridArray
from .quantile import (CunnaneGridModel, CunnaneTransformer, EquidistantCdfMatcher, QmGridModel, QuantileMapper,
                       QuantileMapperGridModel, QuantileMappingReressor, TrendAwareQuantileMappingRegressor)
from .trend import LinearTrendTransformer
from .zscore import ZScoreGridModel, ZScoreRegressor

__all__ = [
    "AnalogRegression",
    "BcsdPrecipitation",
    "BcsdTemperature",
    "PointWiseDownscaler",
    "PureAnalog",
    "MONTH_GROUPER",
    "DAY_GROUPER",
    "PaddedDOYGrouper",
    "GridArray",
    "GridDataset",
    "BcsdGridModel",
    "AnalogGridModel",
    "QuantileMappingReressor", "TrendAwareQuantileMappingRegressor",
    "QuantileMapper",
    "EquidistantCdfMatcher",
    "QmGridModel",
    "CunnaneTransformer",
    "CunnaneGridModel",
    "QuantileMapperGridModel",
    "PureRegression",
    "LinearTrendTransformer",
    "RegressionGridModel",
    "ZScoreRegressor",
    "ZScoreGridModel",
    "GroupedRegressor",
    "GroupedGridModel",
    "PiecewiseLinearRegression",
    "ArrmGridModel",
    "arrm_breakpoints",
    "Regridder",
    "InterpolatedGridArray",
    "ConservativeRemapper",
    "RemappedGridArray",
    "cell_bounds",
    "ResampledGridArray",
    "GridResample",
    "time_bins",
    "DisaggregatedGridArray",
    "time_map",
    "GridGroupBy",
    "GroupReducedGridArray",
    "GroupAppliedGridArray",
    "group_labels",
    "GridRolling",
    "RolledGridArray",
    "TimeQuantileGridArray",
    "GridCondition",
    "SpellGridArray",
    "GridComparison",
    "SkillGridArray",
    "DistributionGridArray",
    "ConstructedAnalogs",
    "ConstructedGridArray",
    "LocalizedAnalogs",
    "LocalizedGridArray",
]
__version__ = "0.1.0"
