from .controller import Controller, ControllerFactory
from .mppi import MPPI, MPPIFactory
from .ilqr import IterativeLQR, IterativeLQRFactory
from .lqr import LQR, LQRFactory, FiniteHorizonLQR, InfiniteHorizonLQR

__all__ = ["Controller", "ControllerFactory", "MPPI", "MPPIFactory", "IterativeLQR",
           "IterativeLQRFactory", "LQR", "LQRFactory", "FiniteHorizonLQR", "InfiniteHorizonLQR"]
