"""Model families (L6 math spec): L2 logistic regression, least squares and the squared-hinge L2-SVM."""
from .losses import (LEAST_SQUARES, LOGISTIC, LOSS_NAMES, SQUARED_HINGE, UpdateRule, is_classification,
                     least_squares_grad, logistic_grad, logistic_loss, mse, roc_auc, squared_hinge_grad,
                     squared_hinge_loss, worker_grad)
