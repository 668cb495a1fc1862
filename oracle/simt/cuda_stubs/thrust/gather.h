// thrust/gather.h -- TEST INFRASTRUCTURE (oracle/simt): see simt_algorithms.h
#pragma once
#include "simt_algorithms.h"
