"""dq4ml — an MI355X-native data-quality + machine-learning tabular pipeline engine with the
Spark API surface of the ``net.jgp.labs.sparkdq4ml`` lab.

    from net.jgp.labs.sparkdq4ml_amd import SparkSession, callUDF, VectorAssembler, LinearRegression
"""
from .sql.session import SparkSession
from .sql.dataframe import DataFrame, Row
from .sql.column import Column
from .sql.functions import callUDF, call_udf, col, lit, udf, when, expr, coalesce
from .sql.window import Window, WindowSpec
from .sql.types import DataTypes, StructType, StructField
from .models.linalg import Vectors, DenseVector, SparseVector, Vector
from .models.feature import VectorAssembler, Imputer, ImputerModel
from .models.regression import (LinearRegression, LinearRegressionModel,
                                LinearRegressionTrainingSummary)
from .models.glm import (GeneralizedLinearRegression, GeneralizedLinearRegressionModel,
                         GeneralizedLinearRegressionSummary, GeneralizedLinearRegressionTrainingSummary)
from .models.tuning import (ParamGridBuilder, CrossValidator, CrossValidatorModel, TrainValidationSplit,
                            TrainValidationSplitModel)
from .dq.rules import MinimumPriceDataQualityUdf, PriceCorrelationDataQualityUdf, IqrRule

__version__ = "0.1.0"

__all__ = [
    "SparkSession", "DataFrame", "Row", "Column", "callUDF", "call_udf", "col", "lit", "udf", "when",
    "expr", "coalesce", "DataTypes", "StructType", "StructField", "Vectors", "DenseVector",
    "SparseVector", "Vector", "VectorAssembler", "LinearRegression", "LinearRegressionModel",
    "LinearRegressionTrainingSummary", "MinimumPriceDataQualityUdf", "PriceCorrelationDataQualityUdf",
    "ParamGridBuilder", "CrossValidator", "CrossValidatorModel", "TrainValidationSplit",
    "TrainValidationSplitModel", "Imputer", "ImputerModel", "IqrRule", "Window", "WindowSpec",
    "GeneralizedLinearRegression", "GeneralizedLinearRegressionModel", "GeneralizedLinearRegressionSummary",
    "GeneralizedLinearRegressionTrainingSummary",
]
