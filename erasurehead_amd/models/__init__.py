"""Model families (L6 math spec): L2 logistic regression, least squares and the squared-hinge L2-SVM."""
from .losses import (LEAST_SQUARES, LOGISTIC, LOSS_CHOICES, LOSS_NAMES, SOFTMAX, SQUARED_HINGE, UpdateRule, accuracy,
                     cv_fold_mask, cv_grad,
                     is_classification, is_multiclass, least_squares_grad, logistic_grad, logistic_loss, mse,
                     ovr_grad, ovr_labels, ovr_loss, roc_auc,
                     softmax_grad, softmax_loss, softmax_unpack, squared_hinge_grad, squared_hinge_loss, worker_grad)
